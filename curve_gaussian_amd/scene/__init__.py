from .dataset_io import default_seed_bounds, edge_vote_point_cloud  # noqa: F401
from .gaussian_curve_model import GaussianCurveModel, Scene, initialize_bezier_curves  # noqa: F401
