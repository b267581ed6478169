from .homography import find_homography_dlt, find_homography_dlt_iterated  # noqa: F401
from .conversions import denormalize_pixel_coordinates, normalize_pixel_coordinates  # noqa: F401
