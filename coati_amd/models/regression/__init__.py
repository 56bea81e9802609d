"""Mirror of coati.models.regression: property regressors on embeddings (property_head.py).  The deterministic part of the reference's
DUE regressor is here -- the FC-ResNet feature extractor with a linear last layer, its fit, and a fused inference kernel
(include/coati_screen.h) -- the GP head and its uncertainty are not (gpytorch / due are not dependencies)."""
from .property_head import PropertyHead, fit_property_head  # noqa: F401
