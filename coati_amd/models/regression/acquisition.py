"""An acquisition of a GPHead as ONE scalar per row with a gradient with respect to the embedding: what uncertainty-aware guided ascent
climbs.

    objective = gp.acquisition("lcb", beta=2.0)             # mean - 2 std of output 0
    values, grad = objective.value_and_grad(vectors)        # [n, 1], [n, input_dim]: one fused kernel (include/coati_acq.h, csrc/gp_grad.hip)
    guided_ascent(start, objective, steps=..., anchor=...)  # coati_amd/generative/coati_guide.py, unchanged
    objective.fused(x)                                      # the same scalar as a differentiable function of x

A bare GPHead has P means and one shared variance and does not say which scalar to climb (its value_and_grad keeps refusing); this object
says it: one output, one of ACQUISITIONS.  The outputs share one variance, so an acquisition that combines several outputs' uncertainties is
out of scope.  There is no CPU fallback; GPHead.reference_acq_grad restates the kernel in torch."""
import torch

from .gp_head import ACQUISITIONS, GPHead
from .property_head import unit_input_chain


class AcquisitionObjective:
    """kind: "mean" (the GP mean, which is not the extractor's linear output), "ucb" = mean + beta std, "lcb" = mean - beta std, "ei" = the
    expected improvement over `best` (required).  output: the one output index it reads.  include_noise: std includes noise_var.  The
    values are acquisition_values(mean[:, output], std[:, output], kind, beta, best) on the kernel's own mean and var."""

    has_input_gradient = True
    num_outputs = 1

    def __init__(self, gp, kind="ucb", beta=1.0, best=None, output=0, include_noise=False):
        if not isinstance(gp, GPHead):
            raise TypeError("AcquisitionObjective: gp must be a GPHead")
        if kind not in ACQUISITIONS:
            raise ValueError(f"AcquisitionObjective: kind={kind!r} is not one of {ACQUISITIONS}")
        output = int(output)
        if not 0 <= output < gp.num_outputs:
            raise ValueError(f"AcquisitionObjective: output={output} outside 0 .. {gp.num_outputs - 1}")
        if kind == "ei" and best is None:
            raise ValueError("AcquisitionObjective: kind 'ei' needs best=, the value to improve on")
        if kind in ("ucb", "lcb") and not float(beta) >= 0.0:
            raise ValueError(f"AcquisitionObjective: beta={beta} must not be negative")
        self.gp, self.kind, self.beta, self.output, self.include_noise = gp, kind, float(beta), output, bool(include_noise)
        self.best = None if best is None else float(best)

    device = property(lambda self: self.gp.device)
    input_dim = property(lambda self: self.gp.input_dim)
    input_dim_padded = property(lambda self: self.gp.input_dim_padded)
    unit_input = property(lambda self: self.gp.unit_input)

    def prepare(self, vectors):
        return self.gp.prepare(vectors)

    def operands(self):
        """(wm [P], kappa, var_add, mode, best) of coati_head_gp_grad: wm = e_output; kappa = +-beta y_scale[output] (ucb, lcb), y_scale[output]
        (ei), 0 (mean); var_add = noise_var if include_noise; mode 1 for ei"""
        gp = self.gp
        wm = torch.zeros(gp.num_outputs, dtype=torch.float32)
        wm[self.output] = 1.0
        scale = float(gp.y_scale[self.output])
        kappa = {"mean": 0.0, "ucb": self.beta * scale, "lcb": -self.beta * scale, "ei": scale}[self.kind]
        return wm, kappa, (gp.noise_var if self.include_noise else 0.0), (1 if self.kind == "ei" else 0), (self.best if self.kind == "ei" else 0.0)

    def acq_rows(self, x16, row_scale=None):
        """(mean, var, acq, g) of GPHead.acq_rows on prepared rows with this objective's operands"""
        wm, kappa, var_add, mode, best = self.operands()
        return self.gp.acq_rows(x16, wm, kappa, var_add, mode, best, row_scale)

    def predict_rows(self, x16):
        """[n, 1] f32: the acquisition of prepared rows"""
        return self.acq_rows(x16)[2][:, None]

    def predict(self, vectors):
        """[n, 1] f32 on the head's device: the acquisition value (the kernel on prepare(vectors))"""
        with torch.no_grad():
            return self.predict_rows(self.prepare(vectors))

    def _row_scale(self, cotangent, n):
        """None, [1] or [n, 1] -> None or [n] f32 on the head's device"""
        if cotangent is None:
            return None
        c = torch.as_tensor(cotangent).detach().to(device=self.device, dtype=torch.float32)
        if c.dim() == 1 and c.shape[0] == 1:
            return c.expand(n).contiguous()
        if c.dim() == 2 and tuple(c.shape) == (n, 1):
            return c[:, 0].contiguous()
        raise ValueError(f"AcquisitionObjective: the cotangent must be None, [1] or [{n}, 1], got {tuple(c.shape)}")

    def value_and_grad(self, vectors, cotangent=None):
        """(values [n, 1], grad [n, input_dim]) f32 on the head's device: predict(vectors) and the gradient of cotangent * values with
        respect to the vectors, one kernel call.  PropertyHead.value_and_grad's contract: the gradient does not see the rounding of the
        input to bf16; with unit_input the chain through the normalisation is unit_input_chain, in f32 torch."""
        x = torch.as_tensor(vectors)
        if x.dim() == 1:
            x = x[None]
        with torch.no_grad():
            x16 = self.prepare(x)
            _, _, acq, g = self.acq_rows(x16, self._row_scale(cotangent, x16.shape[0]))
            g = g[:, :self.input_dim]
            if self.unit_input:
                g = unit_input_chain(g, x.detach().to(device=self.device, dtype=torch.float32))
            return acq[:, None], g.contiguous()

    def fused(self, x):
        """predict(x) [n, 1] as a differentiable function of x [n, input_dim] (models/autograd_funs/property.py): the backward is one
        kernel call with grad_output as the row scale.  Gradients flow to x ONLY."""
        from ..autograd_funs.property import acquisition_fused
        return acquisition_fused(x, self)
