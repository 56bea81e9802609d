"""The likelihood of a token row as a differentiable function of the injected embedding: what the reference gets for free from
autograd through e3gnn_smiles_clip_e2e.hclip_and_tokens_to_likelihood (clip_e2e.py:634-665), on the engine's forward-only scoring path
and its inputs-only backward (Engine.score / Engine.score_grad), and the same for COATI2's embedding behind coati_to_token
(Engine.score_coati2 / Engine.score_grad_coati2)."""
import torch


class HclipLikelihood(torch.autograd.Function):
    """nll [B] = Engine.score(tokens, y_next, h_clip=hclip, rows=rows); the gradient reaches `hclip` [B, E] only -- the model's parameters
    are constants here.

    forward runs the scoring path and keeps nothing of the engine's: its workspace is shared, and any engine call between forward and
    backward carves it again.  backward therefore runs the forward once more inside Engine.score_grad, with grad_output as the
    per-sequence weights; a caller who never calls .backward() pays for the scoring call alone."""

    @staticmethod
    def forward(ctx, hclip: torch.Tensor, engine, tokens: torch.Tensor, y_next: torch.Tensor, rows=None):
        ctx.engine, ctx.rows = engine, rows
        ctx.save_for_backward(hclip, tokens, y_next)
        return engine.score(tokens, y_next, h_clip=hclip, rows=rows)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        hclip, tokens, y_next = ctx.saved_tensors
        _, dh = ctx.engine.score_grad(tokens, y_next, hclip, weights=grad_output, rows=ctx.rows)
        return dh.to(hclip.dtype), None, None, None, None


def hclip_likelihood(hclip, engine, tokens, y_next, rows=None):
    return HclipLikelihood.apply(hclip, engine, tokens, y_next, rows)


class HcoatiLikelihood(torch.autograd.Function):
    """The COATI2 twin of HclipLikelihood: nll [B] = Engine.score_coati2(tokens, y_next, h_coati=hcoati, rows=rows) with coati_to_token of
    `hcoati` [B, E] injected; the gradient reaches `hcoati` only.  forward keeps nothing of the engine's; backward runs
    Engine.score_grad_coati2 with grad_output as the per-sequence weights."""

    @staticmethod
    def forward(ctx, hcoati: torch.Tensor, engine, tokens: torch.Tensor, y_next: torch.Tensor, rows=None):
        ctx.engine, ctx.rows = engine, rows
        ctx.save_for_backward(hcoati, tokens, y_next)
        return engine.score_coati2(tokens, y_next, h_coati=hcoati, rows=rows)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        hcoati, tokens, y_next = ctx.saved_tensors
        _, dh = ctx.engine.score_grad_coati2(tokens, y_next, hcoati, weights=grad_output, rows=ctx.rows)
        return dh.to(hcoati.dtype), None, None, None, None


def hcoati_likelihood(hcoati, engine, tokens, y_next, rows=None):
    return HcoatiLikelihood.apply(hcoati, engine, tokens, y_next, rows)
