"""The full COATI2 shape (FULL of tests/test_gpu_coati2.py, enc_to_coati = "swiglu_resnet") with seeded weights that need neither a
checkpoint nor the reference: tests/golden/gen_golden_coati2_likelihood.py loads them into the reference's model, the GPU tests into
the engine, and tests/golden/coati2_likelihood_golden.npz stores per-parameter checksums of them instead of the 38 M numbers."""
import math

import torch

FULL = dict(n_layer_xformer=12, n_hidden_xformer=512, embed_dim=512, n_head=16, n_seq=250, n_tok=4266)
SEED = 512


def full_param_shapes(cfg=FULL):
    """(name, shape) of every parameter in the reference's state_dict key order (the causal-mask buffers left out)"""
    C, E, V = cfg["n_hidden_xformer"], cfg["embed_dim"], cfg["n_tok"]
    out = [("xformer.emb.tok_emb.weight", (V, C))]
    for l in range(cfg["n_layer_xformer"]):
        p = f"xformer.transformer.h.{l}."
        out += [(p + "ln_1.weight", (C,)), (p + "ln_1.bias", (C,)), (p + "attn.c_attn.weight", (3 * C, C)), (p + "attn.c_attn.bias", (3 * C,)),
                (p + "attn.c_proj.weight", (C, C)), (p + "attn.c_proj.bias", (C,)), (p + "ln_2.weight", (C,)), (p + "ln_2.bias", (C,)),
                (p + "mlpf.0.weight", (4 * C, C)), (p + "mlpf.0.bias", (4 * C,)), (p + "mlpf.2.weight", (C, 4 * C)), (p + "mlpf.2.bias", (C,))]
    out += [("xformer.transformer.ln_f.weight", (C,)), ("xformer.transformer.ln_f.bias", (C,)), ("xformer.lm_head.weight", (V, C))]
    for head, d_in in (("smiles_to_coati", C), ("coati_to_token", E)):
        p = head + ".net."
        out += [(p + "0.weight", (d_in,)), (p + "0.bias", (d_in,)), (p + "2.weight", (2 * E, d_in)), (p + "2.bias", (2 * E,)),
                (p + "4.weight", (E, E)), (p + "4.bias", (E,))]
    return out


def _is_layernorm(name):
    return ".ln_" in name or ".net.0." in name


def full_weights(cfg=FULL, seed=SEED):
    """name -> f32 CPU tensor, parameter i drawn from its own generator seeded seed + i: the embedding N(0, 1), matrices
    U(+-1/sqrt(fan_in)), LayerNorm weights 1 + 0.1 N(0, 1) and biases 0.1 N(0, 1), Linear biases U(+-1/sqrt(fan_in)) of their matrix"""
    shapes = full_param_shapes(cfg)
    fan_in = {n: s[1] for n, s in shapes if len(s) == 2}
    out = {}
    for i, (name, shape) in enumerate(shapes):
        g = torch.Generator().manual_seed(seed + i)
        if name.endswith("tok_emb.weight"):
            v = torch.randn(shape, generator=g)
        elif len(shape) == 2:
            v = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(shape[1])
        elif _is_layernorm(name):
            v = (1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(shape, generator=g)
        else:
            v = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in[name[: -len("bias")] + "weight"])
        out[name] = v
    return out


def checksums(weights, names):
    """(sum, abs-sum) per name, accumulated in float64"""
    return ([float(weights[n].double().sum()) for n in names], [float(weights[n].double().abs().sum()) for n in names])
