"""A property head's prediction as a differentiable function of the embedding, on the head's two kernels: coati_head_eval forward
(PropertyHead.predict_rows), coati_head_grad backward (PropertyHead.grad_rows).  With hclip_likelihood / hcoati_likelihood
(likelihood.py) this lets a property term and a likelihood term stand in one torch objective over the embedding."""
import torch

from ..regression.property_head import unit_input_chain


class HeadFused(torch.autograd.Function):
    """values [n, P] = head.predict(x); the gradient reaches `x` [n, input_dim] only -- the head's parameters are constants here and
    receive no gradient (fit a head with its forward()).

    forward runs the evaluation kernel and keeps x alone.  backward is one coati_head_grad call on the rows prepared again, with
    grad_output as the cotangent (the kernel repeats the forward for the ReLU decisions; nothing of them is kept in memory between the
    two calls), then the chain of unit_input in f32 torch.  The gradient is that of the function predict() computes on the prepared
    rows: it does not see the rounding of x to bf16."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, head):
        ctx.head = head
        ctx.save_for_backward(x)
        return head.predict(x)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        (x,) = ctx.saved_tensors
        head = ctx.head
        with torch.no_grad():
            _, g = head.grad_rows(head.prepare(x), grad_output.to(device=head.device, dtype=torch.float32))
            g = g[:, :head.input_dim]
            if head.unit_input:
                g = unit_input_chain(g, x.detach().to(device=head.device, dtype=torch.float32))
        return g.to(device=x.device, dtype=x.dtype).reshape(x.shape), None


def head_fused(x, head):
    return HeadFused.apply(x, head)


class AcquisitionFused(torch.autograd.Function):
    """values [n, 1] = objective.predict(x) for an AcquisitionObjective (models/regression/acquisition.py); the gradient reaches `x`
    [n, input_dim] only.  backward is one coati_head_gp_grad call (objective.value_and_grad with grad_output as the row scale, the chain
    of unit_input included); nothing is kept between the two calls but x."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, objective):
        ctx.objective = objective
        ctx.save_for_backward(x)
        return objective.predict(x)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        (x,) = ctx.saved_tensors
        _, g = ctx.objective.value_and_grad(x, grad_output)
        return g.to(device=x.device, dtype=x.dtype).reshape(x.shape), None


def acquisition_fused(x, objective):
    return AcquisitionFused.apply(x, objective)
