from .matching import match_mnn, match_nn, match_smnn, match_snn  # noqa: F401
