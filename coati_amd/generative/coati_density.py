"""coati.generative.coati_density (coati/generative/coati_density.py:13-76): a multivariate normal fitted batch by batch to the
embeddings of SMILES strings.  The embeddings come from the packed-row encode; the MVN and its SGD steps are torch on the encoder's
device (E <= 512: plumbing).  The reference's quirks are kept: only the diagonal and lower-triangle parameters are optimised (the mean
stays zero), SGD at lr 5e-3, the entropy printed per batch, an early return below entropy_limit and None otherwise."""
from typing import Iterable, Union

import torch
from torch.distributions.multivariate_normal import MultivariateNormal

from ..common.util import batch_indexable
from . import coati_purifications as _P


def _batch_embeds(batch, encoder, tokenizer, canon_smiles=None):
    """embeddings [n, E] of the batch's strings that canonicalise and tokenize (the others are skipped, as the reference does)"""
    canon = _P._canon_fn(canon_smiles)
    rows = []
    for S in batch:
        c = _P._canonical(canon, S)
        row = None if c is None else _P._token_row_or_none(tokenizer, c)
        if row is not None:
            rows.append(row)
    if not rows:
        return None
    with torch.no_grad():
        return _P._embed_token_rows(encoder, tokenizer, rows)


def estimate_density_batchwise(iterable: Iterable[str], encoder, tokenizer, batch_size: int = 1024, epochs: int = 10,
                               entropy_limit: float = -100, canon_smiles=None) -> Union[MultivariateNormal, None]:
    """Fits N(0, L L^T), L = diag(d * d) + strictly-lower tri, by SGD on the mean negative log-likelihood of each batch's embeddings.
    Returns the distribution as soon as a batch's entropy (that mean NLL) is below entropy_limit, else None after `epochs` passes.
    A batch with no usable string is skipped."""
    E, dev = encoder.embed_dim, encoder.device
    mean_param = torch.nn.Parameter(torch.zeros(E, device=dev))
    sqrt_diag_param = torch.nn.Parameter(0.5 * torch.ones(E, device=dev))
    tril = torch.tril_indices(E, E, offset=-1, device=dev)
    lower_tri_param = torch.nn.Parameter(torch.zeros(tril.shape[1], device=dev))

    def build_distribution(sq_diag, lower):
        L = torch.diag(sq_diag * sq_diag)
        L[tril[0], tril[1]] = lower
        return MultivariateNormal(mean_param, scale_tril=L)

    optimizer = torch.optim.SGD([sqrt_diag_param, lower_tri_param], lr=5e-3)
    for _ in range(epochs):
        for batch in batch_indexable(iterable, batch_size):
            emb = _batch_embeds(batch, encoder, tokenizer, canon_smiles)
            if emb is None:
                continue
            distribution = build_distribution(sqrt_diag_param, lower_tri_param)
            entropy = -distribution.log_prob(emb).mean()
            value = float(entropy.detach().cpu().item())
            print(f"entropy: {value:.4f}")
            if value < entropy_limit:
                return distribution
            optimizer.zero_grad()
            entropy.backward()
            optimizer.step()
    return None
