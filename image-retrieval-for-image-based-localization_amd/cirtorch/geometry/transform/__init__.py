from .pyramid import PyrDown, ScalePyramid, pyrdown  # noqa: F401
