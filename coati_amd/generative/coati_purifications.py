"""coati.generative.coati_purifications (coati/generative/coati_purifications.py): embed SMILES, purify embeddings, decode until valid.

Same function names, parameters and defaults as the reference, plus two batched forms (purify_vectors, force_decode_valid_batches).
rdkit is not a dependency: validity and canonical form come from `canon_smiles` (str -> str; raising or returning None = invalid), the
identity by default -- Chem.CanonSmiles, or MolToSmiles(MolFromSmiles(s)), with rdkit.  Every function takes canon_smiles=None, which
falls back to this module's attribute, so `coati_purifications.canon_smiles = Chem.CanonSmiles` once lets reference code run unchanged.
embed_points takes `mol_to_atoms_coords` (str -> (atoms, coords)) the same way.

Device work: embeddings go through the packed-row encode (coati_engine_encode_packed), decodes through hclip_to_2d_batch
(hcoati_to_2d_batch on a COATI2 model: an extension, the reference has no COATI2 path here), and the batched purification's means
through coati_group_mean_rows.  The host logic -- drop rules, deduplication, tie-break, fallbacks -- is plain Python
(purification_plan, most_frequent_valid) so that it can be checked without a GPU."""
from collections import Counter
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

canon_smiles: Optional[Callable[[str], str]] = None        # None: the identity
mol_to_atoms_coords: Optional[Callable] = None             # str -> (atoms [A], coords [A, 3]); needed by embed_points

DECODE_ROW_CAP = 2048        # rows per decode call of the batched forms: the KV cache is ~ 4 MB per row at the grande shape (16 layers, 250 positions)
ENCODE_ROW_CAP = 1024        # molecules per packed encode call
FORCE_DECODE_CHUNK = 32      # force_decode_valid: attempts drawn per decode call


def _canon_fn(fn):
    fn = fn if fn is not None else canon_smiles
    return fn if fn is not None else (lambda s: s)


def _canonical(fn, s):
    """fn(s), or None when it raises / returns None / s is not a string"""
    if not isinstance(s, str):
        return None
    try:
        c = fn(s)
    except Exception:
        return None
    return c if isinstance(c, str) else None


def _token_row(tokenizer, smi):
    """ids of [SMILES]<smi>[STOP] (tokenize_text's failures raise: an unknown piece, more than n_seq tokens)"""
    return list(tokenizer.tokenize_text("[SMILES]" + smi + "[STOP]", pad=False))


def _token_row_or_none(tokenizer, smi):
    try:
        return _token_row(tokenizer, smi)
    except Exception:
        return None


def _is_coati2(encoder):
    return hasattr(encoder, "hcoati_to_2d_batch")


def _pad_id(encoder, tokenizer):
    eng = getattr(encoder, "engine", None)
    return int(eng.cfg.pad_token) if eng is not None else int(getattr(tokenizer, "pad_token", 0))


def _embed_token_rows(encoder, tokenizer, rows: List[List[int]]) -> torch.Tensor:
    """embeddings [n, E] f32 on the encoder's device of token rows (lists of ids ending in [STOP]): packed encode calls of at most
    ENCODE_ROW_CAP rows.  An encoder without an engine gets the padded rows through its own encode_tokens."""
    pad = _pad_id(encoder, tokenizer)
    eng = getattr(encoder, "engine", None)
    outs = []
    for lo in range(0, len(rows), ENCODE_ROW_CAP):
        chunk = rows[lo:lo + ENCODE_ROW_CAP]
        T = max(len(r) for r in chunk)
        tok = torch.full((len(chunk), T), pad, dtype=torch.long)
        for i, r in enumerate(chunk):
            tok[i, :len(r)] = torch.tensor(r, dtype=torch.long)
        outs.append(_embed_padded(encoder, tokenizer, tok, pad) if eng is not None else encoder.encode_tokens(tok.to(encoder.device), tokenizer))
    return torch.cat(outs) if len(outs) > 1 else outs[0]


def _embed_padded(encoder, tokenizer, tok: torch.Tensor, pad: int) -> torch.Tensor:
    """Engine.encode(rows=...) of host token rows [n, T] (rows1 counted here, on the host)"""
    encoder._sync_tokens(tokenizer)
    T = tok.shape[1]
    live = (tok != pad).to(torch.int64) * torch.arange(1, T + 1, dtype=torch.int64)
    lengths = live.amax(dim=1)
    T = max(int(lengths.max()), 1)
    tok = tok[:, :T].contiguous()
    eng = encoder.engine
    h, _ = eng.encode(tok.to(eng.device), rows=int(lengths.sum()))
    err = int(eng.scal[6:7].view(torch.int32).item())
    if err & 1:
        raise RuntimeError("Some smiles in the batch do not have stop tokens. Did some tokenizations fail?")
    if err & 2:
        raise RuntimeError("packed rows: the row count differs from what the device found in the tokens")
    return h


def _decode_batch(encoder, H: torch.Tensor, tokenizer, generator=None, slots=None, grammar=None) -> List[str]:
    fn = encoder.hcoati_to_2d_batch if _is_coati2(encoder) else encoder.hclip_to_2d_batch
    kw = {} if generator is None else {"generator": generator}
    if grammar is not None:    # (coati_amd.grammar.SmilesGrammar: syntax-constrained decoding)
        kw["grammar"] = grammar
    if slots is not None:
        kw["slots"] = slots
    return list(fn(H, tokenizer, **kw))


def decode_most_likely(model, vectors: torch.Tensor, tokenizer, beams: int = 4, grammar=None):
    """The `beams` most likely SMILES of every row of vectors [N, E] with their log-likelihoods, best first: per vector a list of
    (smiles, log_likelihood) from beam search (hclip_to_2d_beam, hcoati_to_2d_beam on COATI2) -- the deterministic counterpart of
    drawing samples and keeping the most frequent one.  grammar (coati_amd.grammar.SmilesGrammar): only syntactically closable
    continuations are ranked; the log-likelihoods are then renormalised over the admitted tokens (Engine.beam_search)."""
    fn = model.hcoati_to_2d_beam if _is_coati2(model) else model.hclip_to_2d_beam
    V = vectors if vectors.dim() == 2 else vectors.reshape(1, -1)
    return fn(V, tokenizer, beams=beams, **({} if grammar is None else {"grammar": grammar}))


def _decode_repeated(encoder, V: torch.Tensor, tokenizer, n_rep: int, generator=None, slots=None, grammar=None) -> List[Optional[List[str]]]:
    """n_rep decodes of every row of V [N, E], as few decode calls as DECODE_ROW_CAP allows (whole vectors per call).  Per vector the
    list of its n_rep strings in sample order, or None when its decode call raised.
    slots (a number; default None = the chunked calls): ONE streamed call of all N * n_rep rows on that many cache slots
    (Engine.generate_stream: a row that has stopped hands its slot to the next one, so the cache holds `slots` rows whatever N is)."""
    N = V.shape[0]
    if slots is not None:
        try:
            got = _decode_batch(encoder, V.repeat_interleave(n_rep, dim=0), tokenizer, generator, slots=int(slots), grammar=grammar)
            assert len(got) == N * n_rep
            return [got[i * n_rep:(i + 1) * n_rep] for i in range(N)]
        except Exception:
            return [None] * N
    per_call = max(1, DECODE_ROW_CAP // max(n_rep, 1))
    out: List[Optional[List[str]]] = []
    for lo in range(0, N, per_call):
        hi = min(N, lo + per_call)
        H = V[lo:hi].repeat_interleave(n_rep, dim=0)
        try:
            got = _decode_batch(encoder, H, tokenizer, generator, grammar=grammar)
            assert len(got) == H.shape[0]
            out += [got[i * n_rep:(i + 1) * n_rep] for i in range(hi - lo)]
        except Exception:
            out += [None] * (hi - lo)
    return out


def _decode_like_one(encoder, V: torch.Tensor, tokenizer, k: int, generator=None, grammar=None) -> List[str]:
    """k independent draws from the distribution of hclip_to_2d(V) (hcoati_to_2d on COATI2) in one decode call.  hclip_to_2d injects
    h_token[0] -- for a 1-D V its first channel, a scalar spread over the [UNK] row --, and so does this."""
    if getattr(encoder, "engine", None) is None:
        one = encoder.hcoati_to_2d if _is_coati2(encoder) else encoder.hclip_to_2d
        kw = {} if generator is None else {"generator": generator}
        if grammar is not None:
            kw["grammar"] = grammar
        return [one(V, tokenizer, **kw) for _ in range(k)]
    h = V.to(encoder.device, torch.float32)
    if h.dim() == 2:
        return _decode_batch(encoder, h[:1].expand(k, -1).contiguous(), tokenizer, generator, grammar=grammar)
    from ..models.encoding.clip_e2e import injection_prefix
    encoder._sync_tokens(tokenizer)
    h2 = h.reshape(1, -1)
    h_token = encoder.engine.token_head(h2) if _is_coati2(encoder) else encoder.special_tokens_from_clip(h2)
    payload = h_token[0, 0].expand(k, h_token.shape[1]).contiguous()
    gen = encoder.xformer.generate_top_k_with_inj_batch(prefix=injection_prefix(tokenizer, "[SMILES]", False), stop_token=tokenizer.stop_token,
                                                        inv_temp=2, k=100, pad_token=tokenizer.pad_token, inj_token=tokenizer.unk_token,
                                                        inj_payload=payload, generator=generator, **({} if grammar is None else {"grammar": grammar}))
    return [tokenizer.decode(t, special=False) for t in gen]


# ---- host logic ------------------------------------------------------------------------------------------------------------------
@dataclass
class PurificationPlan:
    """What the purification of N vectors encodes and averages.  strings / rows: the distinct canonical strings that tokenize, in
    first-seen order, and their token rows; members[g]: (index into strings, multiplicity) of vector g's kept decodes, in first-seen
    order (empty: nothing survived, the vector is returned unchanged); failed[g]: its decode call raised.  canon_calls: how many
    times the canonicaliser ran (once per distinct raw string)."""
    strings: List[str] = field(default_factory=list)
    rows: List[List[int]] = field(default_factory=list)
    members: List[List[tuple]] = field(default_factory=list)
    failed: List[bool] = field(default_factory=list)
    canon_calls: int = 0

    def expanded(self, g):
        """vector g's kept strings with their repeats (the reference's rows, as a multiset)"""
        return [self.strings[u] for u, c in self.members[g] for _ in range(c)]


def purification_plan(decoded: List[Optional[List[str]]], tokenizer, canon=None) -> PurificationPlan:
    """purify_vector's drop rules over the decodes of N vectors (coati_purifications.py:80-93): a string that fails canonicalisation or
    tokenization is dropped.  Deduplicated first by the raw string (one canonicaliser call each), then by the canonical one (one
    tokenization each)."""
    canon = _canon_fn(canon)
    plan = PurificationPlan()
    raw_to_u, canon_to_u = {}, {}
    for strings in decoded:
        plan.failed.append(strings is None)
        counts = {}
        for S in strings or []:
            u = raw_to_u.get(S) if isinstance(S, str) else -1
            if u is None:
                c = _canonical(canon, S)
                plan.canon_calls += 1
                if c is None:
                    u = -1
                elif c in canon_to_u:
                    u = canon_to_u[c]
                else:
                    row = _token_row_or_none(tokenizer, c)
                    u = -1 if row is None else len(plan.strings)
                    if row is not None:
                        plan.strings.append(c)
                        plan.rows.append(row)
                    canon_to_u[c] = u
                raw_to_u[S] = u
            if u >= 0:
                counts[u] = counts.get(u, 0) + 1
        plan.members.append(list(counts.items()))
    return plan


def most_frequent_valid(strings: Optional[List[str]], canon=None) -> Optional[str]:
    """force_decode_valid_batch's pick (coati_purifications.py:136-150): the canonical forms of the valid strings in decode order, and
    the most frequent of them -- on a tie the one whose first occurrence comes first (np.argmax of the counts).  None: nothing valid."""
    canon = _canon_fn(canon)
    slist = [c for c in (_canonical(canon, S) for S in (strings or [])) if c is not None]
    if not slist:
        return None
    counts = Counter(slist)
    best = max(counts.values())
    return next(s for s in slist if counts[s] == best)


# ---- the reference's functions -----------------------------------------------------------------------------------------------------
def embed_points(s: str, encoder, mol_to_atoms_coords=None) -> torch.Tensor:
    """coati_purifications.py:11-24: encode_points of one molecule's conformer -> [1, E] on the encoder's device."""
    fn = mol_to_atoms_coords if mol_to_atoms_coords is not None else globals()["mol_to_atoms_coords"]
    if fn is None:
        raise RuntimeError("embed_points needs mol_to_atoms_coords (str -> (atoms, coords)): pass mol_to_atoms_coords=... or set "
                           "coati_purifications.mol_to_atoms_coords")
    atoms, coords = fn(s)
    with torch.no_grad():
        return encoder.encode_points(torch.as_tensor(atoms, device=encoder.device).unsqueeze(0).float(),
                                     torch.as_tensor(coords, device=encoder.device).unsqueeze(0).float()).detach().clone()


def embed_smiles(s: str, encoder, tokenizer, canon_smiles=None) -> torch.Tensor:
    """coati_purifications.py:26-40: the embedding [E] of the canonical form of s.  An invalid SMILES raises ValueError, a tokenization
    failure the tokenizer's error."""
    c = _canonical(_canon_fn(canon_smiles), s)
    if c is None:
        raise ValueError(f"embed_smiles: {s!r} is not a valid SMILES string")
    with torch.no_grad():
        return _embed_token_rows(encoder, tokenizer, [_token_row(tokenizer, c)])[0]


def embed_smiles_batch(smiles_list: List[str], encoder, tokenizer) -> torch.Tensor:
    """coati_purifications.py:42-49: embeddings [B, E] of the strings as given (no canonicalisation), through the tokenizer's batch
    encode and the packed-row encode.  A string that does not tokenize raises as tokenize_text does."""
    texts = ["[SMILES]" + s + "[STOP]" for s in smiles_list]
    if not hasattr(tokenizer, "encode_rows"):
        rows = [list(tokenizer.tokenize_text(t, pad=False)) for t in texts]
        with torch.no_grad():
            return _embed_token_rows(encoder, tokenizer, rows)
    tok, lens = tokenizer.encode_rows(texts)
    for i in (lens < 0).nonzero().flatten().tolist():
        tokenizer.tokenize_text(texts[i], pad=True)            # raises the reference's error
    outs = []
    with torch.no_grad():
        for lo in range(0, len(texts), ENCODE_ROW_CAP):
            n = lens[lo:lo + ENCODE_ROW_CAP]
            chunk = tok[lo:lo + ENCODE_ROW_CAP, :int(n.max())]
            outs.append(_embed_padded(encoder, tokenizer, chunk, _pad_id(encoder, tokenizer)) if getattr(encoder, "engine", None) is not None
                        else encoder.encode_tokens(chunk.to(encoder.device), tokenizer))
    return torch.cat(outs) if len(outs) > 1 else outs[0]


def _purify(V: torch.Tensor, plan: PurificationPlan, encoder, tokenizer) -> torch.Tensor:
    """the plan's weighted means [N, E] (coati_group_mean_rows); vectors with nothing kept are V's rows"""
    from .. import ops
    Vd = V.to(encoder.device, torch.float32).contiguous()
    if not plan.strings:
        return Vd.clone()
    emb = _embed_token_rows(encoder, tokenizer, plan.rows)
    idx = [u for m in plan.members for u, _ in m]
    w = torch.tensor([float(c) for m in plan.members for _, c in m], dtype=torch.float32)
    off = [0]
    for m in plan.members:
        off.append(off[-1] + len(m))
    x = emb.index_select(0, torch.tensor(idx, dtype=torch.long, device=emb.device)).contiguous()
    return ops.group_mean_rows(x, off, w=w.to(emb.device), fallback=Vd)


def purify_vector(V: torch.Tensor, encoder, tokenizer, n_rep=128, canon_smiles=None, generator=None, grammar=None) -> torch.Tensor:
    """coati_purifications.py:51-97: decode n_rep copies of V [E]; keep the strings that canonicalise and tokenize; return the mean of
    their embeddings [E].  V itself (the same object) when the decoder raises or nothing is kept.  grammar (here and in the functions
    below; coati_amd.grammar.SmilesGrammar): the decodes are syntax-constrained, so no draw is spent on an unclosed string."""
    with torch.no_grad():
        decoded = _decode_repeated(encoder, V.reshape(1, -1).to(encoder.device, torch.float32), tokenizer, n_rep, generator,
                                   grammar=grammar)
        plan = purification_plan(decoded, tokenizer, canon_smiles)
        if plan.failed[0] or not plan.members[0]:
            return V
        return _purify(V.reshape(1, -1), plan, encoder, tokenizer)[0]


def purify_vectors(V: torch.Tensor, encoder, tokenizer, n_rep=128, canon_smiles=None, generator=None, grammar=None) -> torch.Tensor:
    """purify_vector of every row of V [N, E] -> [N, E]: one decode of the N * n_rep rows (calls of at most DECODE_ROW_CAP rows), the
    distinct molecules encoded once on packed rows, and per vector the multiplicity-weighted mean of its molecules' embeddings
    (coati_group_mean_rows).  Given the same decoded strings, row g equals purify_vector(V[g]) to rounding."""
    assert V.dim() == 2, "purify_vectors: V [N, E]"
    with torch.no_grad():
        decoded = _decode_repeated(encoder, V.to(encoder.device, torch.float32), tokenizer, n_rep, generator, grammar=grammar)
        return _purify(V, purification_plan(decoded, tokenizer, canon_smiles), encoder, tokenizer)


def force_decode_valid(V: torch.Tensor, encoder, tokenizer, max_attempts: int = 2000, canon_smiles=None, generator=None,
                       grammar=None) -> str:
    """coati_purifications.py:100-119: the first valid decode of V (as decoded, not canonicalised), or "C" after max_attempts attempts.
    Attempts are drawn FORCE_DECODE_CHUNK per decode call and taken in sample order: the distribution of the reference's loop, not its
    random stream.  A decode call that raises spends its attempts."""
    canon = _canon_fn(canon_smiles)
    done = 0
    while done < max_attempts:
        k = min(FORCE_DECODE_CHUNK, max_attempts - done)
        try:
            with torch.no_grad():
                cands = _decode_like_one(encoder, V, tokenizer, k, generator, grammar)
        except Exception:
            cands = []
        for S in cands[:k]:
            if _canonical(canon, S) is not None:
                return S
        done += k
    return "C"


def force_decode_valid_batch(V: torch.Tensor, encoder, tokenizer, batch_size: int = 128, max_attempts: int = 4, canon_smiles=None,
                             generator=None, grammar=None) -> str:
    """coati_purifications.py:122-154: up to max_attempts decodes of batch_size copies of V [E]; the most frequent valid canonical string
    of the first attempt that has one (ties: first in decode order), "C" when none does."""
    return force_decode_valid_batches(V.reshape(1, -1), encoder, tokenizer, batch_size=batch_size, max_attempts=max_attempts,
                                      canon_smiles=canon_smiles, generator=generator, grammar=grammar)[0]


def force_decode_valid_batches(V: torch.Tensor, encoder, tokenizer, batch_size: int = 128, max_attempts: int = 4, canon_smiles=None,
                               generator=None, grammar=None) -> List[str]:
    """force_decode_valid_batch of every row of V [N, E] -> N strings.  Each attempt decodes the vectors still unresolved together
    (calls of at most DECODE_ROW_CAP rows); each vector follows the reference's rule."""
    assert V.dim() == 2, "force_decode_valid_batches: V [N, E]"
    canon = _canon_fn(canon_smiles)
    N = V.shape[0]
    out: List[Optional[str]] = [None] * N
    todo = list(range(N))
    Vd = V.to(encoder.device, torch.float32) if getattr(encoder, "device", None) is not None else V
    for _ in range(max_attempts):
        if not todo:
            break
        with torch.no_grad():
            decoded = _decode_repeated(encoder, Vd[todo], tokenizer, batch_size, generator, grammar=grammar)
        still = []
        for g, strings in zip(todo, decoded):
            pick = most_frequent_valid(strings, canon)
            if pick is None:
                still.append(g)
            else:
                out[g] = pick
        todo = still
    return [s if s is not None else "C" for s in out]
