"""Mirror of coati.models.regression: property regressors on embeddings.  The reference's DUE regressor is an FC-ResNet feature extractor
with a Gaussian-process head on inducing points: the extractor with a linear last layer, its fit and its fused kernels
(include/coati_screen.h, include/coati_guide.h) are property_head.py; the GP head with its predictive uncertainty, fitted in closed form
(no gpytorch / due) and evaluated in the same fused pass (include/coati_gp.h), is gp_head.py."""
from .property_head import PropertyHead, fit_property_head  # noqa: F401
from .gp_head import GPHead, acquisition_values, fit_gp_head  # noqa: F401
