from .pyramid import ScalePyramid  # noqa: F401
