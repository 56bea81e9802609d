"""Mirror of coati.models.regression: property regressors on embeddings.  The reference's DUE regressor is an FC-ResNet feature extractor
with a Gaussian-process head on inducing points: the extractor with a linear last layer, its fit and its fused kernels
(include/coati_screen.h, include/coati_guide.h) are property_head.py; the GP head with its predictive uncertainty, fitted in closed form
(no gpytorch / due) and evaluated in the same fused pass (include/coati_gp.h), is gp_head.py; an acquisition of it as one scalar with a gradient with respect to the
embedding (include/coati_acq.h), what uncertainty-aware guided ascent climbs, is acquisition.py."""
from .property_head import PropertyHead, fit_property_head  # noqa: F401
from .gp_head import ACQUISITIONS, GPHead, acquisition_values, fit_gp_head  # noqa: F401
from .acquisition import AcquisitionObjective  # noqa: F401
