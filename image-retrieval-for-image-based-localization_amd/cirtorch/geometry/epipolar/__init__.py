from .fundamental import (compute_correspond_epilines, find_fundamental, normalize_points,  # noqa: F401
                          normalize_transformation)
from .metrics import sampson_epipolar_distance, symmetrical_epipolar_distance  # noqa: F401
