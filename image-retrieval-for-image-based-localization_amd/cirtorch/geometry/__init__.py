from .homography import find_homography_dlt, find_homography_dlt_iterated  # noqa: F401
