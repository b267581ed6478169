from .spatial_soft_argmax import ConvQuadInterp3d, ConvSoftArgmax3d, conv_quad_interp3d  # noqa: F401
