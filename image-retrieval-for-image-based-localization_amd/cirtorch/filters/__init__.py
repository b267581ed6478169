from .gaussian import GaussianBlur2d, gaussian_blur2d  # noqa: F401
