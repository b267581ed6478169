from .perspective import project_points, unproject_points  # noqa: F401
