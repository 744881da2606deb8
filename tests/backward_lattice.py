"""Exact checks of the NONLINEAR BACKWARD kernels on lattices (helpers; no GPU needed).

tests/saturated_lattice.py gates the fused forward kernels at zero.  The backward kernels contain the same three nonlinear pieces -- a LayerNorm, a
softmax, a GELU' -- and each has inputs on which the kernels' own float32 arithmetic is exact:

  LayerNorm backward (layernorm_bwd_kernel: rstd = 1.0f / sqrtf(var + 1e-5f)): a row a * s, s a balanced +-1 pattern, C a power of two, a in {16, 32, 64}
      has float32 mean 0, variance a^2 and float32(a^2 + 1e-5) == a^2, so rstd = 1 / a and xhat = +-1 EXACTLY.  With integer dy and odd integer gamma
      every value -- s1, s2, dx, dgamma, dbeta -- is a small multiple of 1 / (a C): exact in any summation order.  (a = 8 fails: half an ulp of 64 is 3.8e-6.)
  softmax backward (window_attn_bwd_kernel, window_attn_bwd2_kernel, win4_attn_bwd_kernel): equal logits over n = 64 / 32 / 16 keys give P = 1 / n; a
      winner ahead by MARGIN = 104 gives P = 1 and exactly 0 elsewhere; two equal winners give 1 / 2.  With integer dO and v, dP is an integer,
      dot = sum(P dP) and dS = P (dP - dot) are exact, and every product with q, k, dO is a float32 sum of lattice values.
  GELU' (gelu_grad_t): a >= 8 gives exactly 1, a = 0 exactly 1/2 (the sigmoid form: rcp(2), an ulp at most, which the store to T absorbs), a <= -15 exactly 0
      in the erf form; the sigmoid form keeps 2^-80 (1 + a (...)) there because of its clamp (``gelu_residue_bound``: bf16 stores it, f16 flushes it).

The gate is exact_lattice.assert_exact against the DOCUMENTED formula in float64, rounded once to T at each documented rounding point: P and dS as MFMA
operands (8 x 8 kernels, 2-byte types), dq / dk / dvt / dqkv, dc = T(stencil) or T(GEMM) in front of GELU', h = T(GELU(pre)), the cast output of
uf_layernorm_bwd_cast.  float32 outputs are not rounded.  Three single IEEE operations are mirrored: rstd := 1 / a, the query scale of the merged outputs
(one float32 multiply by float32(head_dim^-0.5) on the exact accumulator), DropPath scales (powers of two or 0).  Every condition is asserted on the
float64 reference alone, by the builders below, so tests/test_backward_lattice_reference.py (CPU) and tests/test_gpu_backward_exact.py check the same cases.

The -100 shift mask leaves e = exp(-100), a float32 subnormal that the hardware may keep or flush.  The "uniform" construction is built so that it never
decides a bit: dP - dot = sigma_j m_i with a key sign sigma_j and m_i > 0, k = sigma_j tau_d |k|, q = tau'_d |q|, dO > 0 -- every float32 sum that
receives such a term has a non-zero exact part of one sign (asserted), in which the term disappears.  One-hot and tie cases have leads of 104 or more
everywhere (e is exactly 0), and a caller mask holds -208.
"""
import functools
import math

import torch
import torch.nn.functional as F

import exact_lattice as X
import saturated_lattice as S
from exact_lattice import BF16, F16, F32, PM1, PM2, check_accumulation, check_representable, lattice
from saturated_lattice import MARGIN, gen, pick

KINDS = ("uniform", "onehot", "tie")
CALLER_MASK = -2.0 * MARGIN


def nz(t):
    """-0 -> +0.  Used ONLY behind a GELU' of exactly 0: the float64 value there is a negative number below every subnormal (it rounds to -0 times the
    sign of the gradient) where the erf form returns +0 and the clamped sigmoid form a negative residue: the sign of that zero carries no information"""
    return t + 0.0


def representable(t64, dtype):
    """condition 2 on a tensor that need not be integer: every value is a T value (rounding it to T is the identity)"""
    m = float(t64.abs().max())
    check_representable(t64, dtype, step=m if m > 0 else 1.0)


def check_sum(abs_a, abs_b, step):
    """condition 1 for the contraction a @ b: the largest sum of |terms| of any output, in lattice steps, is below 2^24"""
    return check_accumulation(1, (float((abs_a @ abs_b).max()) / step,))


# ---------------------------------------------------------------------------------------------------------------------------
# window attention backward, 8 x 8 windows (uf_window_attention_bwd, uf_window_attention_bwd_qkv)
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, heads, head_dim, shift, kind, caller mask).  16 x 16 has a plain, a last-column, a last-row and a corner window: means over 64 / 32 / 16 keys.
# "uniform" with shift needs every (query, key) pair unmasked in SOME window (dbias would otherwise be an exact 0 fed by subnormals only): 16 x 16, never
# 8 x 24 (one row of windows: all of them are last-row windows).  8 x 24 with B = 3 is 9 windows.  The caller mask (the MK = true instantiation of the second
# kernel) runs with shift 0.  66 windows of 16 heads: 1024 / 16 = 64 chunks, so two workgroups of every head walk two windows and add their dbias slices.
def _attn_cases():
    cases = []
    for hd, heads in ((16, (1, 4, 2)), (32, (2, 1, 4)), (64, (4, 2, 1))):
        for kind, h in zip(KINDS, heads):
            cases.append((1, 16, 16, h, hd, 0, kind, False))
            cases.append((1, 16, 16, heads[(KINDS.index(kind) + 1) % 3], hd, 4, kind, False))
        cases += [(3, 8, 24, heads[0], hd, 0, "uniform", False), (3, 8, 24, heads[1], hd, 4, "onehot", False), (3, 8, 24, heads[2], hd, 4, "tie", False)]
        cases += [(1, 16, 16, 2, hd, 0, "uniform", True), (1, 16, 16, 2, hd, 0, "onehot", True)]
    cases += [(66, 8, 8, 16, 16, 0, "uniform", False), (66, 8, 8, 16, 16, 0, "tie", False)]
    return cases


ATTN_BWD_CASES = _attn_cases()


def caller_mask64():
    """(2, 64, 64) in {0, -208}: pattern 0 removes the keys of the other x half, pattern 1 those of the other y half: half the keys either way"""
    t = torch.arange(64)
    xh, yh = (t % 8) >= 4, (t // 8) >= 4
    return torch.stack([torch.where(xh[:, None] != xh[None, :], CALLER_MASK, 0.0), torch.where(yh[:, None] != yh[None, :], CALLER_MASK, 0.0)]).double()


def total_mask(n, H, W, shift, caller):
    """(n, 64, 64): the shift mask of window w % nW plus the caller mask w % n_mask, as the kernels index them"""
    sm = S.shift_mask64(H, W, shift)
    m = sm[torch.arange(n) % sm.shape[0]]
    return m if caller is None else m + caller[torch.arange(n) % caller.shape[0]]


def _sigma(heads, g):
    """(heads, 64) key signs, balanced inside every quadrant: the mean of sigma over any union of quadrants (any mask region) is 0"""
    out = torch.zeros(heads, 64, dtype=torch.float64)
    for h in range(heads):
        for grp in S._quadrants():
            p = grp[torch.randperm(16, generator=g)]
            out[h, p[:8]], out[h, p[8:]] = 1.0, -1.0
    return out


def _coded_qk(n, heads, hd, tie, g):
    """q, k of the "onehot" / "tie" kinds: k = a signed Hadamard code times an amplitude, q = A times the code a query selects, A hd = 128.  All selections
    stay inside the query's quadrant (never behind a mask).  onehot, head_dim >= 32: 64 distinct codes per window, any other token of the quadrant selected.
    onehot at head_dim 16: a quadrant holds 8 codes twice, with amplitudes 4 and 1 (the holder with 4 wins by 384).  "tie": codes of HALF the head width on the
    first half of the channels, 8 per quadrant held by two tokens each (4 held by four at head_dim 16) with one amplitude -- equal winners -- and on the second half,
    where q is zero, k rows of their own, so that dq = sum dS k does not cancel.  -> (q, k, winners (n, heads, 64, 64) bool)"""
    codes, A = S.signed_codes(hd), 128 // hd
    q = torch.zeros(n, heads, 64, hd, dtype=torch.float64)
    k = torch.zeros_like(q)
    win = torch.zeros(n, heads, 64, 64, dtype=torch.bool)
    quads = S._quadrants()
    paired = hd == 16
    half = hd // 2
    hcodes, nc = S.signed_codes(half), min(8, half // 2)                                     # "tie": codes per quadrant (8, or 4 at head_dim 16), each held by 16 / nc tokens
    for w in range(n):
        for h in range(heads):
            perm = torch.randperm(2 * half if tie else 2 * hd, generator=g)
            tcode, amp = torch.empty(64, dtype=torch.long), torch.empty(64, dtype=torch.float64)
            for qi, grp in enumerate(quads):
                p = grp[torch.randperm(16, generator=g)]
                if tie:
                    cq = perm[nc * qi:nc * qi + nc]
                    tcode[p] = cq.repeat(16 // nc)
                    amp[p] = torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (nc,), generator=g)].repeat(16 // nc)
                    sel = cq[torch.randint(nc, (16,), generator=g)]                      # the code every query of the quadrant selects
                    q[w, h, p, :half] = (128 // half) * hcodes[sel]
                    win[w, h, p[:, None], p[None, :]] = tcode[p][None, :] == sel[:, None]
                elif paired:
                    cq = perm[8 * qi:8 * qi + 8]
                    tcode[p] = cq.repeat(2)
                    amp[p] = torch.cat([torch.full((8,), 4.0), torch.full((8,), 1.0)]).double()
                    sel = cq[torch.randint(8, (16,), generator=g)]
                    q[w, h, p] = A * codes[sel]
                    win[w, h, p[:, None], p[None, :]] = (tcode[p][None, :] == sel[:, None]) & (amp[p] == 4.0)[None, :]
                else:
                    cq = perm[16 * qi:16 * qi + 16]
                    tcode[p] = cq
                    amp[p] = torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (16,), generator=g)]
                    tgt = (torch.arange(16) + torch.randint(1, 16, (16,), generator=g)) % 16        # another token of the quadrant
                    q[w, h, p] = A * codes[cq[tgt]]
                    win[w, h, p, p[tgt]] = True
            if tie:                                                                      # the winners' k rows differ in the half q does not see: dq stays live
                k[w, h, :, :half] = hcodes[tcode] * amp[:, None]
                k[w, h, :, half:] = pick(PM2, (64, hd - half), int(torch.randint(1 << 30, (1,), generator=g)))
            else:
                k[w, h] = codes[tcode] * amp[:, None]
    return q, k, win


def attn_bwd_eval(c, dtype, fault=None, mask=None):
    """The documented backward of the attention core in float64 -- P = softmax(q k^T + bias + mask), dv = P^T dO, dP = dO v^T, dS = P (dP - sum(P dP)),
    dq = dS k, dk = dS^T q, dbias = sum over windows of dS -- with P and dS rounded to T where they are MFMA operands (2-byte types), and optionally ONE
    fault (stand-ins of tests/test_backward_lattice_reference.py).  A probability below 1e-40 (a key behind the -100 shift mask) counts as 0."""
    q, k, v, dO = c["q"], c["k"], c["v"], c["dO"]
    s = q @ k.transpose(2, 3) + c["bias"][None] + (c["mask"] if mask is None else mask)[:, None]
    P = torch.softmax(s, 3)
    P = torch.where(P < 1e-40, torch.zeros_like(P), P)
    dP = dO @ v.transpose(2, 3)
    PdP = P * dP
    dot = (PdP[..., :48] if fault == "dot48" else PdP).sum(3, keepdim=True)
    dS = (P.roll(1, 2) if fault == "p_neighbour" else P) * (dP - dot)
    rt = (lambda t: t.to(dtype).double()) if dtype != F32 else (lambda t: t)
    dSo, Po = rt(dS), rt(P)
    dSb = dS.clone()
    if fault == "dbias_second_window":
        dSb[1] = 0.0
    return {"P": P, "dS": dS, "dP": dP, "dot": dot[..., 0], "dq": dSo @ k, "dk": dSo.transpose(2, 3) @ (q * math.sqrt(c["hd"]) if fault == "dk_unscaled_q" else q),
            "dvt": ((Po if fault == "dv_untransposed" else Po.transpose(2, 3)) @ dO).transpose(2, 3).contiguous(), "dbias": dSb.sum(0)}


def merge_heads(t):
    """(n, heads, 64, hd) -> (n * 64, heads * hd)"""
    n, heads, _, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(n * 64, heads * hd)


def qscale32(hd):
    return torch.tensor(float(hd) ** -0.5, dtype=torch.float32)


def scaled_f32(t64, scale32):
    """one float32 multiply on an exact accumulator (asserted to be a float32 value), as the kernels scale dq before the store"""
    t = t64.float()
    assert torch.equal(t.double(), t64), "the accumulator is not a float32 value"
    return t * scale32


def rpb_table_grad64(dbias):
    """(heads, 64, 64) -> (225, heads): the transpose of the gather table[relative_position_index]"""
    heads = dbias.shape[0]
    return torch.zeros(225, heads, dtype=torch.float64).index_add_(0, X.rpb_index(8).reshape(-1), dbias.permute(1, 2, 0).reshape(4096, heads))


@functools.lru_cache(maxsize=None)
def attn_bwd_case(B, H, W, heads, hd, shift, kind, masked):
    """operands (float64 lattice values, exact in every operand type) and the float64 reference; every condition of the header is asserted here"""
    n = B * (H // 8) * (W // 8)
    g = gen(900 + hd + 3 * heads + shift + 11 * KINDS.index(kind) + 5 * int(masked) + H)
    caller = caller_mask64() if masked else None
    assert not (masked and shift), "a pair behind -100 here and -208 everywhere else would feed dbias subnormals only"
    mask = total_mask(n, H, W, shift, caller)
    if kind == "uniform":
        assert shift == 0 or (H // 8 > 1 and W // 8 > 1)
        hq = hd // 2
        sig = _sigma(heads, g)
        b_, u_ = pick((3, 4), (n, heads, 1, hd), 901 + hd), pick((1, 2) if hd <= 32 else (1,), (n, heads, 1, hd), 902 + hd)
        v = b_ + sig[None, :, :, None] * u_
        dO = pick((1, 2), (n, heads, 64, hd), 903 + hd + heads)
        q, k = torch.zeros(n, heads, 64, hd, dtype=torch.float64), torch.zeros(n, heads, 64, hd, dtype=torch.float64)
        q[..., :hq] = pick(PM1, (1, heads, 1, hq), 904 + hd) * pick((1, 2), (n, heads, 64, hq), 905 + hd)            # disjoint channel supports: q k^T = 0
        k[..., hq:] = sig[None, :, :, None] * pick(PM1, (1, heads, 1, hd - hq), 906 + hd) * pick((1, 2), (n, heads, 64, hd - hq), 907 + hd)
        bias = pick((-2, -1, 0, 1, 2), (heads, 64, 1), 908 + heads).expand(heads, 64, 64).contiguous()                # a constant per query row keeps the logits equal
        winners = (mask > -50.0)[:, None].expand(n, heads, 64, 64)
    else:
        q, k, winners = _coded_qk(n, heads, hd, kind == "tie", g)
        v = pick((-3, -2, -1, 1, 2, 3), (n, heads, 64, hd), 911 + hd + heads)
        live = torch.rand(n, heads, 64, hd, generator=g).argsort(3) < (4 if hd == 16 else 8)                          # 8 (4) live channels per token and head: |dP| <= 48 (24)
        dO = pick(PM2, (n, heads, 64, hd), 912 + hd + heads) * live
        bias = (torch.ones(heads, 64, 64, dtype=torch.float64) if kind == "tie"
                else pick((-2, -1, 0, 1, 2), (225, heads), 913 + heads)[X.rpb_index(8)].permute(2, 0, 1).contiguous())
    c = {"q": q, "k": k, "v": v, "vt": v.transpose(2, 3).contiguous(), "dO": dO, "dO_rows": merge_heads(dO), "bias": bias, "mask": mask, "caller": caller,
         "n": n, "hd": hd, "heads": heads, "kind": kind}
    r = attn_bwd_eval(c, F32)
    # ---- conditions, on the reference alone
    s = q @ k.transpose(2, 3) + bias[None] + mask[:, None]
    top = s.max(3, keepdim=True).values
    assert torch.equal(s == top, winners), "the winners are not the intended keys"
    n_win = winners.sum(3, keepdim=True)
    lead = (top - torch.where(winners, torch.full_like(s, -1e9), s).max(3, keepdim=True).values)
    shift_only = (S.shift_mask64(H, W, shift)[torch.arange(n) % ((H // 8) * (W // 8))] < 0)[:, None]                  # keys 100 behind: covered by the sign structure
    behind = torch.where(winners | (shift_only & (kind == "uniform")), torch.full_like(s, 1e9), top - s)
    assert float(behind.min()) >= MARGIN and (kind == "uniform" or float(lead.min()) >= MARGIN), (float(behind.min()), float(lead.min()))
    assert torch.equal(r["P"], winners.double() / n_win), "the documented softmax is not the lattice value"
    got_n = set(n_win.unique().tolist())
    if kind == "uniform":
        assert got_n == ({32} if masked else ({64} if not shift else {16, 32, 64}))
        m = (dO * u_).sum(3)                                                                                           # (n, heads, 64): dP - dot = sigma_j m_i
        assert bool((m > 0).all()) and torch.equal(r["dS"], winners * (sig[None, :, None, :] * m[..., None] / n_win))
        assert bool((r["dot"] > 0).all()) and bool((r["dvt"] > 0).all())
        assert bool((r["dq"][..., hq:] != 0).all()) and bool((r["dq"][..., :hq] == 0).all()) and bool((r["dk"][..., :hq] != 0).all()) and bool((r["dk"][..., hq:] == 0).all())
        ever = winners.any(0)
        assert bool(ever.all()) or masked, "a pair masked in every window"
        assert bool(((r["dbias"] != 0) == ever).all()), "a dbias entry that cancels to zero"
    elif kind == "onehot":
        assert got_n == {1}
        assert not bool(r["dS"].any()) and not bool(r["dq"].any()) and not bool(r["dk"].any()) and not bool(r["dbias"].any())
        assert torch.equal(r["dvt"].transpose(2, 3), winners.double().transpose(2, 3) @ dO) and bool(r["dvt"].any())     # dv: the dO rows of the queries that selected the key
    else:
        m = 4 if hd == 16 else 2
        assert got_n == {m}
        tot = (r["dP"] * winners).sum(3, keepdim=True)
        assert torch.equal(r["dS"], winners * (m * r["dP"] - tot) / (m * m))                                            # two winners: +-(dP_a - dP_b) / 4
        assert float((r["dS"] != 0).any(3).double().mean()) > 0.5, "the winners hold the same dP too often"
        assert not bool(r["dq"][..., :hd // 2].any()) and bool(r["dq"][..., hd // 2:].any()) and bool(r["dk"].any())      # dq is live where the winners' k rows differ
    assert float((r["dot"] != 0).double().mean()) >= 0.5, "dot must be live on at least half the rows"
    for t in (BF16, F16):
        representable(r["P"], t)
        representable(r["dS"], t)
    check_sum(dO.abs(), v.abs().transpose(2, 3), 1.0)
    step = 1.0 / 4096
    check_sum(r["dS"].abs(), k.abs(), step)
    check_sum(r["dS"].abs().transpose(2, 3), q.abs(), step)
    check_sum(r["P"].abs().transpose(2, 3), dO.abs(), 1.0 / 64)
    check_accumulation(1, (float(r["dS"].abs().sum(0).max()) / step,))
    for key in ("dq", "dk", "dvt", "dbias"):
        assert torch.equal(r[key].float().double(), r[key]), key
    dqkv_q = scaled_f32(merge_heads(r["dq"]), qscale32(hd))
    c.update(ref=r, dqkv=torch.cat([dqkv_q.double(), merge_heads(r["dk"]), merge_heads(r["dvt"].transpose(2, 3))], 1), dtable=rpb_table_grad64(r["dbias"]),
             n_win=n_win, flat=lambda t: t.reshape(n * heads, t.shape[2], t.shape[3]))
    check_accumulation(1, (float(rpb_table_grad64(r["dbias"].abs()).max()) / step,))
    return c


def attn_bwd_emulate_f32(c, dtype):
    """float32 emulation of the kernels' arithmetic: max-subtracted exp, inv = 1 / sum, P = e inv, dot = sum(P dP), dS = P (dP - dot), P and dS rounded to T
    as operands (2-byte types), float32 sums"""
    q, k, v, dO = (c[key].float() for key in ("q", "k", "v", "dO"))
    s = q @ k.transpose(2, 3) + c["bias"].float()[None] + c["mask"].float()[:, None]
    e = torch.exp(s - s.max(3, keepdim=True).values)
    P = e * (1.0 / e.sum(3, keepdim=True))
    dP = dO @ v.transpose(2, 3)
    dS = P * (dP - (P * dP).sum(3, keepdim=True))
    rt = (lambda t: t.to(dtype).float()) if dtype != F32 else (lambda t: t)
    return {"dq": rt(dS) @ k, "dk": rt(dS).transpose(2, 3) @ q, "dvt": (rt(P).transpose(2, 3) @ dO).transpose(2, 3), "dbias": dS.sum(0)}


# ---------------------------------------------------------------------------------------------------------------------------
# window attention backward, 4 x 4 windows (uf_window4_attention_bwd): raster q | k | v rows, the kernel applies head_dim^-0.5, P and dS stay float32
# ---------------------------------------------------------------------------------------------------------------------------
ATTN4_BWD_CASES = [(B, H, W, heads, hd, kind) for kind in KINDS for (B, H, W, heads, hd) in ((1, 8, 8, 2, 16), (3, 4, 12, 1, 32), (1, 8, 8, 5, 32), (2, 8, 4, 8, 16))]


def attn4_bwd_eval(c, fault=None):
    q, k, v, dO, sc = c["q"], c["k"], c["v"], c["dO"], float(c["scale"])
    s = (q @ k.transpose(2, 3)) * sc + c["bias"][None]
    P = torch.softmax(s, 3)
    P = torch.where(P < 1e-40, torch.zeros_like(P), P)
    dP = dO @ v.transpose(2, 3)
    PdP = P * dP
    dot = (PdP[..., :12] if fault == "dot48" else PdP).sum(3, keepdim=True)
    dS = (P.roll(1, 2) if fault == "p_neighbour" else P) * (dP - dot)
    return {"P": P, "dS": dS, "dot": dot[..., 0], "dq": dS @ k, "dk": dS.transpose(2, 3) @ q, "dv": (P if fault == "dv_untransposed" else P.transpose(2, 3)) @ dO}


def rpb4_table_grad64(dscore):
    """(n, heads, 16, 16) -> (49, heads)"""
    t = torch.arange(16)
    ent = ((t[:, None] // 4) - (t[None, :] // 4) + 3) * 7 + ((t[:, None] % 4) - (t[None, :] % 4) + 3)
    heads = dscore.shape[1]
    return torch.zeros(49, heads, dtype=torch.float64).index_add_(0, ent.reshape(-1), dscore.sum(0).permute(1, 2, 0).reshape(256, heads))


@functools.lru_cache(maxsize=None)
def attn4_bwd_case(B, H, W, heads, hd, kind):
    n, C = B * (H // 4) * (W // 4), heads * hd
    g = gen(950 + hd + heads + H + KINDS.index(kind))
    scale = qscale32(hd)
    codes = S.signed_codes(hd)
    v = pick((-3, -2, -1, 1, 2, 3), (n, heads, 16, hd), 951 + hd + heads)
    dO = pick(PM2, (n, heads, 16, hd), 952 + hd + heads)
    q = torch.zeros(n, heads, 16, hd, dtype=torch.float64)
    k = torch.zeros_like(q)
    winners = torch.zeros(n, heads, 16, 16, dtype=torch.bool)
    if kind == "uniform":
        hq = hd // 2
        q[..., :hq] = pick(PM2, (n, heads, 16, hq), 953 + hd)
        k[..., hq:] = pick(PM2, (n, heads, 16, hd - hq), 954 + hd)
        tab = torch.full((heads, 49), 3.0, dtype=torch.float64)
        winners[:] = True
    else:
        for w in range(n):
            for h in range(heads):
                if kind == "tie":                                              # 8 codes of half the head width, each held by two tokens with one amplitude
                    half = hd // 2
                    hc = S.signed_codes(half)
                    cq = torch.randperm(2 * half, generator=g)[:8]
                    p = torch.randperm(16, generator=g)
                    tcode, amp = torch.empty(16, dtype=torch.long), torch.empty(16, dtype=torch.float64)
                    tcode[p] = cq.repeat(2)
                    amp[p] = torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (8,), generator=g)].repeat(2)
                    sel = cq[torch.randint(8, (16,), generator=g)]
                    q[w, h, :, :half] = 2 * S.Q_GAIN4 * hc[sel]
                    winners[w, h] = tcode[None, :] == sel[:, None]
                    k[w, h, :, :half] = hc[tcode] * amp[:, None]
                    k[w, h, :, half:] = pick(PM2, (16, hd - half), int(torch.randint(1 << 30, (1,), generator=g)))   # k rows of their own where q is zero: dq stays live
                    continue
                else:
                    tcode = torch.randperm(2 * hd, generator=g)[:16]
                    amp = torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (16,), generator=g)]
                    tgt = (torch.arange(16) + torch.randint(1, 16, (16,), generator=g)) % 16
                    q[w, h] = S.Q_GAIN4 * codes[tcode[tgt]]
                    winners[w, h, torch.arange(16), tgt] = True
                k[w, h] = codes[tcode] * amp[:, None]
        tab = torch.ones(heads, 49, dtype=torch.float64) if kind == "tie" else pick((-2, -1, 0, 1, 2), (heads, 49), 955 + heads)
    bias = S.rpb4_dense(tab)
    c = {"q": q, "k": k, "v": v, "dO": dO, "bias": bias, "tab": tab, "scale": scale, "n": n, "C": C, "heads": heads, "hd": hd, "kind": kind}
    r = attn4_bwd_eval(c)
    s = (q @ k.transpose(2, 3)) * float(scale) + bias[None]
    top = s.max(3, keepdim=True).values
    n_win = winners.sum(3, keepdim=True)
    behind = torch.where(winners, torch.full_like(s, 1e9), top - s)
    assert float(behind.min()) >= MARGIN + 4 and torch.equal(r["P"], winners.double() / n_win)
    assert set(n_win.unique().tolist()) == {"uniform": {16}, "onehot": {1}, "tie": {2}}[kind]
    if kind == "onehot":
        assert not bool(r["dS"].any()) and not bool(r["dq"].any()) and not bool(r["dk"].any()) and bool(r["dv"].any())
    else:
        assert float((r["dS"] != 0).any(3).double().mean()) > 0.5 and bool(r["dk"].any())
        assert bool(r["dq"].any())
    assert float((r["dot"] != 0).double().mean()) >= 0.5
    step = 1.0 / 256
    check_sum(dO.abs(), v.abs().transpose(2, 3), 1.0)
    check_sum(r["dS"].abs(), k.abs(), step)
    check_sum(r["dS"].abs().transpose(2, 3), q.abs(), step)
    check_sum(r["P"].transpose(2, 3), dO.abs(), 1.0 / 16)
    rows = S.window4_rows(B, H, W).reshape(-1)
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(n * 16, C)                   # noqa: E731
    qkv, do_rows = torch.zeros(B * H * W, 3 * C, dtype=torch.float64), torch.zeros(B * H * W, C, dtype=torch.float64)
    qkv[rows], do_rows[rows] = torch.cat([merge(q), merge(k), merge(v)], 1), merge(dO)
    dqkv = torch.zeros(B * H * W, 3 * C, dtype=torch.float64)
    dqkv[rows] = torch.cat([scaled_f32(merge(r["dq"]), scale).double(), scaled_f32(merge(r["dk"]), scale).double(), merge(r["dv"])], 1)
    dtable = rpb4_table_grad64(r["dS"])
    check_accumulation(1, (float(rpb4_table_grad64(r["dS"].abs()).max()) / step,))
    c.update(ref=r, qkv=qkv, dO_rows=do_rows, dqkv=dqkv, dscore=r["dS"], dtable=dtable)
    return c


def attn4_bwd_emulate_f32(c):
    q, k, v, dO = (c[key].float() for key in ("q", "k", "v", "dO"))
    s = (q @ k.transpose(2, 3)) * c["scale"] + c["bias"].float()[None]
    e = torch.exp(s - s.max(3, keepdim=True).values)
    P = e * (1.0 / e.sum(3, keepdim=True))
    dP = dO @ v.transpose(2, 3)
    dS = P * (dP - (P * dP).sum(3, keepdim=True))
    return {"dq": (dS @ k) * c["scale"], "dk": (dS.transpose(2, 3) @ q) * c["scale"], "dv": P.transpose(2, 3) @ dO, "dS": dS}


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward (uf_layernorm_bwd, uf_layernorm_bwd_fused, uf_layernorm_bwd_cast)
# ---------------------------------------------------------------------------------------------------------------------------
LN_AMPS = (16, 32, 64)
LN_WIDTHS = [16, 32, 64, 128, 256, 512, 1024]
LN_GRID = 2048                                   # LN_BWD_MAX_BLOCKS in csrc/uf_bwd.hip: above LN_GRID * rows_per_workgroup rows the grid-stride loop takes a second trip
# plain uf_layernorm_bwd, (C, rows): 130 rows are no multiple of the 64 / 32 / 16 / 8 / 4 rows of a workgroup (C = 16 ... 128, 256 and up); the other three
# exceed the grid (C = 16: 64 rows per workgroup, C = 64: 16, C = 256: 4) by a ragged block
LN_PLAIN_CASES = [(C, 130) for C in LN_WIDTHS] + [(16, 64 * LN_GRID + 37), (64, 16 * LN_GRID + 5), (256, 4 * LN_GRID + 3)]
DROPS = (0.0, 2.0, 1.0)


def drops(B):
    """per-image DropPath scales (0, 2, 1), repeated for more than three images"""
    return (DROPS * ((B + 2) // 3))[:B]


# the fused / cast forms on maps of whole windows: (B, H, W, windowed, shift, add, dy as f32, cast (None / "token" / "window"), cast_shift, cast scales)
LN_FUSED_CONFIGS = [
    (3, 8, 24, True, 4, True, False, None, 0, False),
    (1, 16, 16, True, 0, False, True, None, 0, False),
    (3, 8, 24, False, 0, True, True, None, 0, False),
    (3, 8, 24, False, 0, True, False, "window", 4, True),          # LN2 of a block: token-order dz, the window-order copy with the DropPath scales of the attention branch
    (3, 8, 24, True, 4, True, False, "token", 0, True),            # LN1 of a block: window-order dxn, the token-order copy for the preceding block
    (1, 16, 16, True, 4, False, False, "window", 0, False),
    (1, 16, 16, False, 0, False, False, "token", 0, False),
]


# one configuration above the grid (C = 16: 64 rows per workgroup, 9 maps of 128 x 128 = 147456 rows > 64 x 2048): the second trip of the grid-stride loop with
# window-order T dy, the residual gradient and the window-order cast output with scales -- the per-trip index arithmetic of those forms
LN_FUSED_BIG = (16, (9, 128, 128, True, 4, True, False, "window", 0, True))


def rows_per_workgroup(C):
    return 256 // min(C // 4, 64)


@functools.lru_cache(maxsize=None)
def ln_bwd_case(C, M, seed=0):
    x, s = S.balanced_rows(M, C, 1000 + C + seed, amps=LN_AMPS)
    a = x.abs().amax(1, keepdim=True)
    a32 = a.float()
    assert torch.equal((a32 * a32 + torch.tensor(S.LN_EPS, dtype=F32)), a32 * a32), "eps must disappear in float32(a^2 + eps)"
    gamma = pick((-3, -1, 1, 3), (C,), 1001 + C)
    dy, add = lattice((M, C), PM2, 1002 + C + seed), lattice((M, C), PM2, 1003 + C + seed)
    g_ = dy * gamma
    assert bool((g_.sum(1) != 0).any()) and bool(((g_ * s).sum(1) != 0).any()), "s1 and s2 must be live"
    assert float((g_.sum(1) != 0).double().mean()) > 0.5 and float(((g_ * s).sum(1) != 0).double().mean()) > 0.5
    # s1, s2: integer sums of |g| <= 6 over C channels; dx = (g - s1 - xhat s2) / a + add in steps of 1 / (64 C): |.| <= 18 / 16 + 2; dgamma / dbeta: |dy| <= 2 over M rows
    check_accumulation(C, (6,))
    check_accumulation(1, (72 * C + 128 * C,))
    check_accumulation(M, PM2)
    return {"x": x, "s": s, "a": a, "gamma": gamma, "dy": dy, "add": add, "C": C, "M": M}


def ln_bwd_eval(c, tok=None, add=False, cast=None, dtype=F32, fault=None):
    """dx (token rows), dgamma, dbeta and the cast output of the documented backward, rstd := 1 / a.  ``tok``: the token of dy row m (window order) or None;
    ``cast`` = (destination row of every TOKEN, per-image scales or None, rows per image).  One optional fault."""
    x, s, a, gamma, dy = c["x"], c["s"], c["a"], c["gamma"], c["dy"]
    M, C = x.shape
    tok = torch.arange(M) if tok is None else tok
    rstd = 1.0 / a[tok]
    xhat = x[tok] * rstd
    g_ = dy * gamma
    s1 = g_.mean(1, keepdim=True)
    s2 = torch.zeros_like(s1) if fault == "s2_dropped" else (g_ * xhat).mean(1, keepdim=True)
    r = (g_ - s1 - xhat * s2) * rstd
    if add:
        r = r + (c["add"] if fault == "add_at_window_row" else c["add"][tok])
    dx = torch.zeros(M, C, dtype=torch.float64)
    dx[tok] = r
    keep = torch.ones(M, dtype=torch.bool)
    if fault == "dgamma_row_lane":
        keep[torch.arange(M) % rows_per_workgroup(C) == 1] = False
    out = {"dx": dx, "dgamma": (dy * xhat)[keep].sum(0), "dbeta": dy[keep].sum(0)}
    if cast is not None:
        dest, scales, hw = cast
        img = torch.arange(M) // hw
        sc = torch.ones(M, dtype=torch.float64) if scales is None else torch.tensor(scales, dtype=torch.float64)[(img + 1) % len(scales) if fault == "cast_scale_neighbour" else img]
        co = torch.zeros(M, C, dtype=torch.float64)
        co[dest[tok]] = r * sc[:, None]
        out["cast"] = co.to(dtype).double() if dtype != F32 else co
    return out


def cast_rows(B, H, W, windowed, shift):
    """destination row of every token in the cast output: its own, or its window-order row"""
    M = B * H * W
    if not windowed:
        return torch.arange(M)
    dest = torch.empty(M, dtype=torch.long)
    dest[X.window_tokens(B, H, W, shift)] = torch.arange(M)
    return dest


def ln_bwd_emulate_f32(c, tok=None, add=False):
    """float32 emulation of layernorm_bwd_kernel, eps included"""
    x, gamma, dy = c["x"].float(), c["gamma"].float(), c["dy"].float()
    M, C = x.shape
    tok = torch.arange(M) if tok is None else tok
    inv = torch.tensor(1.0 / C, dtype=F32)
    xr = x[tok]
    v = xr - xr.sum(1, keepdim=True) * inv
    rstd = 1.0 / torch.sqrt((v * v).sum(1, keepdim=True) * inv + torch.tensor(S.LN_EPS, dtype=F32))
    v = v * rstd
    g_ = dy * gamma
    s1, s2 = g_.sum(1, keepdim=True) * inv, (g_ * v).sum(1, keepdim=True) * inv
    r = (g_ - s1 - v * s2) * rstd
    if add:
        r = r + c["add"].float()[tok]
    dx = torch.zeros(M, C, dtype=F32)
    dx[tok] = r
    return {"dx": dx, "dgamma": (dy * v).sum(0), "dbeta": dy.sum(0)}


# ---------------------------------------------------------------------------------------------------------------------------
# GELU' (uf_gelu_bwd, uf_linear_mul_dgelu, uf_dwconv3x3_mul_dgelu, uf_dwconv3x3_bwd)
# ---------------------------------------------------------------------------------------------------------------------------
POS_MIN, POS_MAX, NEG_MAX = 8, 64, -15
C0, C1 = 1.5957691216, 0.2140610                          # the float32 constants of gelu_grad_t's sigmoid form
CLASS_SHARES = (0.40, 0.25, 0.35)                          # a >= 8, a = 0, a <= -15: each at least a fifth; the negative class (rule (b) in bf16) under 40 %
RULE_B_CAP = 0.40


def neg_min(dtype):
    return -256 if dtype == F32 else -64


def gelu_pre(shape, dtype, seed, classes=(0, 1, 2)):
    """integer pre-activations of the three classes (``classes`` picks a subset), drawn per element"""
    g = gen(seed)
    shares = torch.tensor([CLASS_SHARES[i] for i in classes], dtype=torch.float64)
    cls = torch.tensor(classes)[torch.multinomial(shares / shares.sum(), int(torch.tensor(shape).prod()), replacement=True, generator=g)].reshape(shape)
    pos = torch.randint(POS_MIN, POS_MAX + 1, shape, generator=g).double()
    neg = -torch.randint(-NEG_MAX, -neg_min(dtype) + 1, shape, generator=g).double()
    pre = torch.where(cls == 0, pos, torch.where(cls == 1, torch.zeros(shape, dtype=torch.float64), neg))
    check_classes(pre, dtype, classes)
    return pre


def check_classes(pre64, dtype, classes=(0, 1, 2)):
    pos, zero, neg = pre64 >= POS_MIN, pre64 == 0, pre64 <= NEG_MAX
    assert bool((pos | zero | neg).all()) and float(pre64.max()) <= POS_MAX and float(pre64.min()) >= neg_min(dtype)
    shares = [float(m.double().mean()) for m in (pos, zero, neg)]
    assert all(shares[i] >= 0.2 for i in classes), shares
    assert shares[2] <= RULE_B_CAP, shares
    return shares


def gelu_grad_doc64(a, dtype):
    """the documented derivative in float64: Phi(a) + a phi(a) (erf form, f32) or the derivative of a / (1 + 2^u), u = a (A + B a^2) (2-byte types), written
    as sg (1 + a (1 - sg) (C0 + C1 a^2)) with a sigmoid that does not overflow"""
    if dtype == F32:
        return 0.5 * torch.special.erfc(-a / math.sqrt(2.0)) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    A, B = float(torch.tensor(S.GELU_A, dtype=F32)), float(torch.tensor(S.GELU_B, dtype=F32))
    u = a * (A + B * a * a)
    t = torch.exp2(-u.abs())
    sg = torch.where(u > 0, t / (1.0 + t), 1.0 / (1.0 + t))
    return sg * (1.0 + a * (1.0 - sg) * (C0 + C1 * a * a))


def gelu_grad_lattice(pre64, dtype, skip=None):
    """GELU' of class members: 1, 1/2, 0 -- asserted to be what the documented formula rounds to (float32 for f32 operands; for the 2-byte types the product
    with a gradient of up to 2^11 lattice steps must round to the lattice product).  ``skip``: a class whose GELU' a faulty kernel leaves out (= 1)"""
    gl = torch.where(pre64 >= POS_MIN, 1.0, torch.where(pre64 == 0, 0.5, 0.0)).double()
    doc = gelu_grad_doc64(pre64, dtype)
    if dtype == F32:
        assert torch.equal(nz(doc.float()).double(), gl)
    else:
        assert float((doc - gl).abs().max()) < 2.0 ** -40                     # 2^-40 of a gradient below 2^11: far inside half an ulp of any T value on the lattice
    if skip is not None:
        gl = torch.where([pre64 >= POS_MIN, pre64 == 0, pre64 <= NEG_MAX][skip], torch.ones_like(gl), gl)
    return gl


def gelu_grad_kernel_f32(a32, dtype):
    """float32 emulation of gelu_grad_t, operation by operation"""
    if dtype == F32:
        return 0.5 * (1.0 + torch.erf(a32 * torch.tensor(0.70710678118654752440, dtype=F32))) + a32 * torch.exp(-0.5 * a32 * a32) * torch.tensor(0.39894228040143267794, dtype=F32)
    A, B = torch.tensor(S.GELU_A, dtype=F32), torch.tensor(S.GELU_B, dtype=F32)
    u = torch.clamp(a32 * (a32 * a32 * B + A), max=80.0)
    e = torch.exp2(u)
    sg = 1.0 / (e + 1.0)
    return sg + a32 * e * sg * sg * (torch.tensor(C0, dtype=F32) + torch.tensor(C1, dtype=F32) * a32 * a32)


def gelu_residue_bound(dc64, pre64):
    """rule (b): what the clamp u <= 80 of the sigmoid form leaves of dc * GELU'(a) for a <= -15, doubled"""
    a = pre64.abs()
    return 2.0 * dc64.abs() * 2.0 ** -80 * (1.0 + a * (C0 + C1 * a * a))


def mul_dgelu(dc64, pre64, dtype, skip=None):
    """T(T(dc) * GELU'(pre)): the gradient as stored, times the lattice GELU', stored again"""
    dcT = dc64.to(dtype).double()
    out = dcT * gelu_grad_lattice(pre64, dtype, skip)
    assert float(gelu_residue_bound(dcT, pre64).max()) < 2.0 ** -24 * 0.5, "rule (b) must stay below 2^-24 of the lattice step (1/2)"
    return torch.where(pre64 <= NEG_MAX, nz(out), out)                          # the sign of a zero is dropped behind GELU' = 0 only


GELU_BWD_N = [8 * 3, 64 * 50 * 3, 8 * (256 * 3 + 5)]       # elements: under one workgroup, whole workgroups, a ragged last one


@functools.lru_cache(maxsize=None)
def gelu_bwd_case(n, dtype):
    pre = gelu_pre((n,), dtype, 1100 + n) if n >= 64 else torch.tensor([8, 0, -15, 64, 0, float(neg_min(dtype)), 9, -16] * (n // 8), dtype=torch.float64)
    dy = lattice((n,), (-4, -3, -2, -1, 1, 2, 3, 4), 1101 + n)
    return {"pre": pre, "dy": dy, "dx": mul_dgelu(dy, pre, dtype)}


# (M, N, K, UF_VARIANT): both staging paths where the LDS-DMA one exists, a ragged M, and the 128-column tile (512 tiles of 128 x 128 and more)
LINEAR_DGELU_CASES = [(130, 32, 32, None), (64, 64, 64, None), (130, 96, 128, "gemm_dma=0"), (130, 96, 128, "gemm_dma=1"), X.GEMM_WIDE_TILE_CASE + (None,)]


@functools.lru_cache(maxsize=None)
def linear_dgelu_case(M, N, K, dtype):
    c = dict(X.gemm_case(M, N, K))
    representable(c["P"], dtype)                                                # dc = T(A W^T + bias) rounds nothing
    pre = gelu_pre((M, N), dtype, 1110 + N + K)
    c.update(pre=pre, out=mul_dgelu(c["P"], pre, dtype))
    return c


# (B, H, W, C): 8 x 8 is all border, 16 x 16, 8 x 24 (the walking kernel of the 2-byte types), 8 x 12 / 12 x 12 (W no multiple of 8: the strip form)
DW_BWD_CASES = [(1, 8, 8, 64), (2, 16, 16, 32), (1, 8, 24, 128), (2, 8, 12, 16), (1, 12, 12, 32)]


def dw9_residue_bound(c):
    """(9, C): what the clamp's residue in h = T(GELU(pre)) -- a 2^-80 for a <= -15, which bf16 stores and f16 flushes (its smallest subnormal is 2^-24) -- can add
    to a tap gradient, doubled: 2 x 2^-80 x sum over the pixels of |dc a|.  It disappears in any float32 sum whose exact part is non-zero; where the reference
    is 0 it is all there is"""
    neg = c["pre"] <= NEG_MAX
    return (2.0 * 2.0 ** -80 * (c["dc"].abs() * c["pre"].abs() * neg).sum((0, 1, 2))).expand(9, -1)


@functools.lru_cache(maxsize=None)
def dw_bwd_case(B, H, W, C, dtype):
    """dc in +-1, nine distinct taps per channel; da = T(T(stencil(dc; flipped taps)) GELU'(pre)); dw9 / dbias from h = T(GELU(pre))"""
    g = gen(1120 + C + H + W)
    taps = torch.tensor(S.TAPS, dtype=torch.float64)[torch.rand(C, 9, generator=g).argsort(1)]                        # (C, 9), tap = ky * 3 + kx
    assert all(len(set(r.tolist())) == 9 for r in taps)
    dc = lattice((B, H, W, C), PM1, 1121 + C + H)
    pre = gelu_pre((B, H, W, C), dtype, 1122 + C + W)
    c = {"taps": taps, "w9": taps.t().contiguous(), "w9_flipped": taps.t().flip(0).contiguous(), "dc": dc, "pre": pre}
    c.update(dw_bwd_eval(c, dtype))
    check_accumulation(9, PM1, S.TAPS)
    check_accumulation(B * H * W, (POS_MAX,), PM1)
    assert bool(c["dw9"].any(1).all()) and bool(c["dbias"].any()) and bool(c["da"].any())
    return c


def dw_bwd_eval(c, dtype, fault=None, skip=None):
    """faults: "taps_unflipped" (the stencil of da run with the forward taps), "h_not_gelu" (the tap gradient contracted with the pre-activation)"""
    dc, pre = c["dc"], c["pre"]
    B, H, W, C = dc.shape
    w = c["taps"].reshape(C, 1, 3, 3)
    if fault == "taps_unflipped":
        st = F.conv2d(dc.permute(0, 3, 1, 2), w, None, padding=1, groups=C)
    else:
        st = F.conv_transpose2d(dc.permute(0, 3, 1, 2), w, None, padding=1, groups=C)                                  # dh[y, x] = sum w[ky, kx] dc[y - ky + 1, x - kx + 1]
    st = st.permute(0, 2, 3, 1)
    if dtype != F32:
        representable(st, dtype)
    da = mul_dgelu(st, pre, dtype, skip)
    h = pre if fault == "h_not_gelu" else torch.where(pre >= POS_MIN, pre, torch.zeros_like(pre))                     # T(GELU(pre)): pre, 0, (-)0
    hp = F.pad(h.permute(0, 3, 1, 2), (1, 1, 1, 1))
    dcp = dc.permute(0, 3, 1, 2)
    dw9 = torch.stack([(dcp * hp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3)) for ky in range(3) for kx in range(3)])   # (9, C) tap-major
    return {"stencil": st, "da": da, "dw9": dw9, "dbias": dc.sum((0, 1, 2))}


# ---------------------------------------------------------------------------------------------------------------------------
# the LeFF half of a block (uf_leff_bwd): LN2 -> linear1 -> GELU -> depthwise 3x3 -> GELU -> linear2, recomputed from x1 and differentiated
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, C).  C = 1024 stays out: the block entry points take head_dim 32 and the widest stage of the models is 512
LEFF_BWD_CASES = [(B, H, W, C) for C in (32, 64, 128, 256, 512) for (B, H, W) in ((1, 16, 16), (3, 8, 24))]
B1_POS, B1_NEG = 13.0, -20.0                               # a1 = +-z + b1 with |z| <= 5: [8, 18] or [-25, -15]
STENCIL_MAX = 18 * 20                                      # |stencil(h1)| <= max h1 * sum |BLOCK_TAPS|


def leff_classes(C, dtype):
    """class (0: >= 8, 1: = 0, 2: <= -15) of the linear1 pre-activation a1 and of the stencil output c, per hidden channel.  A channel whose h1 = GELU(a1) is
    live can only put c into class 0 or 2 (through the stencil's bias); a channel with h1 = 0 has c = bias exactly: any class.  bf16 runs the classes 0 and 1
    only (rule (b) of DESIGN.md 2.5: its GELU keeps a residue of the clamp in h1 and g2, which the tap and linear2 gradients would sum)"""
    pat = [(0, 0), (0, 2), (1, 1), (2, 1), (1, 2), (2, 0), (0, 0), (1, 0), (2, 2), (0, 2), (1, 1), (2, 1)] if dtype != BF16 else [(0, 0), (1, 1), (0, 0), (1, 0), (1, 1)]
    idx = torch.arange(4 * C) % len(pat)
    t = torch.tensor(pat)
    return t[idx, 0], t[idx, 1]


def _cls_grad(v64, dtype):
    """lattice GELU' of a stored pre-activation whose class is read from its value"""
    assert bool(((v64 >= POS_MIN) | (v64 == 0) | (v64 <= NEG_MAX)).all())
    doc = gelu_grad_doc64(v64.clamp(min=-300.0), dtype)
    gl = torch.where(v64 >= POS_MIN, 1.0, torch.where(v64 == 0, 0.5, 0.0)).double()
    assert float((doc - gl).abs().max()) < 2.0 ** -40
    return gl


def exact_f32(t64, what):
    assert torch.equal(t64.float().double(), t64), f"{what} is not a float32 value: the kernel's arithmetic would round"
    return t64


@functools.lru_cache(maxsize=None)
def leff_bwd_case(B, H, W, C, dtype, dropped):
    """operands of uf_leff_bwd and the float64 reference of dx1 and the eight gradient tensors, T roundings at z, a1, c, g2, dyT, dc, da1, dz"""
    M, hid = B * H * W, 4 * C
    g = gen(1200 + C + H)
    rt = (lambda t: t.to(dtype).double()) if dtype != F32 else (lambda t: t)
    x1, s = S.balanced_rows(M, C, 1201 + C + H, amps=LN_AMPS)
    a = x1.abs().amax(1, keepdim=True)
    gamma2, beta2 = pick((-3, -1, 1, 3), (C,), 1202 + C), pick((-2, 0, 2), (C,), 1203 + C)
    z = s * gamma2 + beta2
    representable(z, BF16)
    cls1, cls2 = leff_classes(C, dtype)
    w1 = S.sparse_pm1(hid, C, 1204 + C, nnz=1) * (cls1 != 1)[:, None]
    b1 = torch.where(cls1 == 0, B1_POS, torch.where(cls1 == 1, 0.0, B1_NEG)).double()
    a1 = z @ w1.t() + b1
    for k in (0, 1, 2):
        assert bool(((a1 >= POS_MIN, a1 == 0, a1 <= NEG_MAX)[k] == (cls1 == k)[None, :]).all())
    h1 = torch.where(a1 >= POS_MIN, a1, torch.zeros_like(a1))
    taps = torch.tensor(S.BLOCK_TAPS, dtype=torch.float64)[torch.rand(hid, 9, generator=g).argsort(1)]
    jit = torch.randint(3, (hid,), generator=g).double()
    live = cls1 == 0
    bdw = torch.where(cls2 == 0, POS_MIN + jit + STENCIL_MAX * live, torch.where(cls2 == 1, torch.zeros(hid, dtype=torch.float64), NEG_MAX - jit - STENCIL_MAX * live))
    cpre = F.conv2d(h1.reshape(B, H, W, hid).permute(0, 3, 1, 2), taps.reshape(hid, 1, 3, 3), bdw, padding=1, groups=hid).permute(0, 2, 3, 1).reshape(M, hid)
    cT = rt(exact_f32(cpre, "c"))
    for k in (0, 1, 2):
        assert bool(((cT >= POS_MIN, cT == 0, cT <= NEG_MAX)[k] == (cls2 == k)[None, :]).all())
    shares = [float((cls == k).double().mean()) for cls in (cls1, cls2) for k in ((0, 1) if dtype == BF16 else (0, 1, 2))]
    assert min(shares) >= 0.2, shares
    g2 = torch.where(cT >= POS_MIN, cT, torch.zeros_like(cT))
    w2 = S.sparse_pm1(hid, C, 1205 + C, nnz=2).t().contiguous()                                     # (C, 4C): two entries per hidden channel keep dc small
    b2 = lattice((C,), PM2, 1206 + C)
    dy = lattice((M, C), PM2, 1207 + C + H)
    drop = torch.tensor(DROPS[:B] if B == 3 else (2.0,), dtype=torch.float64) if dropped else torch.ones(B, dtype=torch.float64)
    sc = drop.repeat_interleave(H * W)[:, None]
    # ---- backward
    tA = rt(dy * sc)
    gw2, gb2 = tA.t() @ g2, tA.sum(0)
    check_sum(tA.abs().t(), g2.abs(), 1.0)
    dc = rt(rt(tA @ w2) * _cls_grad(cT, dtype))
    st = F.conv_transpose2d(dc.reshape(B, H, W, hid).permute(0, 3, 1, 2), taps.reshape(hid, 1, 3, 3), None, padding=1, groups=hid).permute(0, 2, 3, 1).reshape(M, hid)
    da1 = nz(rt(rt(exact_f32(st, "the input-gradient stencil")) * _cls_grad(a1, dtype)))
    hp = F.pad(h1.reshape(B, H, W, hid).permute(0, 3, 1, 2), (1, 1, 1, 1))
    dcp = dc.reshape(B, H, W, hid).permute(0, 3, 1, 2)
    dw9 = torch.stack([(dcp * hp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3)) for ky in range(3) for kx in range(3)])
    check_accumulation(1, (float(torch.stack([(dcp.abs() * hp[:, :, ky:ky + H, kx:kx + W].abs()).sum((0, 2, 3)) for ky in range(3) for kx in range(3)]).max()) / 0.5,))
    gw1, gb1 = da1.t() @ z, da1.sum(0)
    check_sum(da1.abs().t(), z.abs(), 0.25)
    dz = rt(exact_f32(da1 @ w1, "dz"))
    check_sum(da1.abs(), w1.abs(), 0.25)
    # LN2 backward on dz, plus the residual path dy: every float32 intermediate must be exact, whatever the compiler contracts
    xhat, rstd = s, 1.0 / a
    g_ = dz * gamma2
    s1, s2 = exact_f32(g_.sum(1, keepdim=True), "sum g") / C, exact_f32((g_ * xhat).sum(1, keepdim=True), "sum g xhat") / C
    check_accumulation(1, (float(g_.abs().sum(1).max()) / 0.25,))
    t1 = exact_f32(g_ - s1, "g - s1")
    t2 = exact_f32(t1 - xhat * s2, "g - s1 - xhat s2")
    exact_f32(g_ - xhat * s2, "g - xhat s2")
    dx1 = exact_f32(exact_f32(t2 * rstd, "dx of LN2") + dy, "dx1")
    gn2w, gn2b = (dz * xhat).sum(0), dz.sum(0)
    check_accumulation(1, (float(dz.abs().sum(0).max()) / 0.25,))
    refs = {"dx1": dx1, "norm2_w": gn2w, "norm2_b": gn2b, "w1": gw1, "b1": gb1, "wdw": dw9.t().contiguous().reshape(hid, 1, 3, 3), "bdw": dc.sum(0), "w2": gw2, "b2": gb2}
    for k, v in refs.items():
        assert bool(v.any()), f"{k} is identically zero"
        exact_f32(v, k)
    assert bool((g_.sum(1) != 0).any()) and bool(((g_ * xhat).sum(1) != 0).any())
    sd = {"norm2.weight": gamma2, "norm2.bias": beta2, "mlp.linear1.0.weight": w1, "mlp.linear1.0.bias": b1, "mlp.dwconv.0.weight": taps.reshape(hid, 1, 3, 3),
          "mlp.dwconv.0.bias": bdw, "mlp.linear2.0.weight": w2, "mlp.linear2.0.bias": b2,
          # the attention half is not run by uf_leff_bwd: placeholders of the right shapes
          "norm1.weight": torch.ones(C, dtype=torch.float64), "norm1.bias": torch.zeros(C, dtype=torch.float64), "attn.qkv.to_q.weight": torch.zeros(C, C, dtype=torch.float64),
          "attn.qkv.to_q.bias": torch.zeros(C, dtype=torch.float64), "attn.qkv.to_kv.weight": torch.zeros(2 * C, C, dtype=torch.float64),
          "attn.qkv.to_kv.bias": torch.zeros(2 * C, dtype=torch.float64), "attn.relative_position_bias_table": torch.zeros(225, C // 32, dtype=torch.float64),
          "attn.proj.weight": torch.zeros(C, C, dtype=torch.float64), "attn.proj.bias": torch.zeros(C, dtype=torch.float64)}
    return {"x1": x1, "dy": dy, "drop": drop if dropped else None, "sd": sd, "refs": refs, "a1": a1, "c": cT, "h1": h1, "dc": dc, "da1": da1, "dz": dz, "z": z,
            "taps": taps, "tA": tA, "w2": w2, "w1": w1, "gamma2": gamma2, "s": s, "a": a}


# ---------------------------------------------------------------------------------------------------------------------------
# the attention half of a block (uf_lewin_attn_bwd): LN1 -> q | k | v -> window attention -> projection, recomputed from x and differentiated
# ---------------------------------------------------------------------------------------------------------------------------
def attn_half_cases(dtype):
    """(B, H, W, C, shift, kind, modulator): the saturated block constructions of tests/saturated_lattice.py (head_dim 32).  "onehot" has dS = 0 (the gather and the scatter
    of the rows are observed through dv); "uniform" and "table" have Wq = 0 and bq = 0: dk = 0, dq is live (in "table" on the rows whose entry points outside the window).  f32 runs "uniform" and "table" with LayerNorm
    weight 0, as the forward does (its onehot constructions need xn rounded to T)"""
    out = []
    for C in (32, 64, 128, 256, 512):
        if dtype != F32:
            out += [(1, 16, 16, C, 0, "onehot", False), (1, 16, 16, C, 4, "onehot", C > 32)]
        # f32 (LayerNorm weight 0) needs the modulator: without it every row of xn is the bias, every key of a window equal, and dq = k sum_j dS = 0
        out += [(3, 8, 24, C, 0, "table", True), (1, 16, 16, C, 4, "uniform", True), (3, 8, 24, C, 0, "uniform", dtype == F32)]
    return out


@functools.lru_cache(maxsize=None)
def attn_half_bwd_case(B, H, W, C, shift, kind, use_mod, dtype, dropped):
    """operands of uf_lewin_attn_bwd and the float64 reference of dx and the gradients of norm1, modulator, rpb_table, wqkv / bqkv, wproj / bproj.  Roundings to T:
    xn, q (after the float32 scale), k, v, o, dyw, dO, P and dS (operands), dq (after the scale) | dk | dv, dxn.  ``bounds``: the q rows of wqkv / bqkv under
    "uniform" sum T-rounded multiples of float32(32^-0.5), which is not order-free: (M - 1) 2^-24 sum |terms| (exception (a) of DESIGN.md 2.5)."""
    c = S.block_case(B, H, W, C, shift, kind, use_mod, dtype)
    M, heads = B * H * W, C // 32
    n = M // 64
    rt = (lambda t: t.to(dtype).double()) if dtype != F32 else (lambda t: t)
    heads_of = lambda t: t.reshape(n, 64, heads, 32).permute(0, 2, 1, 3)          # noqa: E731
    tok = c["tok"]
    x = 16.0 * c["x"]                                                              # row amplitudes 16, 32, 64: LayerNorm's output does not change, eps disappears
    a = x.abs().amax(1, keepdim=True)
    assert set(a.unique().tolist()) <= {16.0, 32.0, 64.0}
    xn, P = c["xn"], c["P"]
    q, k, v = heads_of(c["q_plain"].double()), heads_of(P[:, C:2 * C]), heads_of(P[:, 2 * C:])
    mask = total_mask(n, H, W, shift, None)
    wqkv = torch.cat([c["wq"], c["wk"], c["wv"]], 0)
    # the recomputed forward of the op-level kernels (natural-domain softmax on the stored q) saturates like the fused kernel's
    s = q @ k.transpose(2, 3) + c["bias"][None] + mask[:, None]
    top = s.max(3, keepdim=True).values
    Pm = torch.softmax(s, 3)
    winners = Pm > 1e-40
    behind = torch.where(winners | (mask[:, None] < 0), torch.full_like(s, 1e9), top - s)
    assert float(behind.min()) >= MARGIN, float(behind.min())
    assert torch.equal(merge_heads(winners.double() @ v / winners.sum(3, keepdim=True)), c["o"]), "the op-level forward does not reproduce the block's o"
    o = c["o"]
    # ---- backward
    dx1 = lattice((M, C), PM2, 1300 + C + H + shift)
    drop = torch.tensor(DROPS[:B] if B == 3 else (2.0,), dtype=torch.float64) if dropped else torch.ones(B, dtype=torch.float64)
    dyw = rt(dx1[tok] * drop[tok // (H * W)][:, None])
    gwp, gbp = dyw.t() @ o, dyw.sum(0)
    check_sum(dyw.abs().t(), o.abs(), 1.0 / 64)
    dO = rt(exact_f32(dyw @ c["wp"], "dO"))
    ac = {"q": q, "k": k, "v": v, "dO": heads_of(dO), "bias": c["bias"], "mask": mask, "hd": 32}
    ev = attn_bwd_eval(ac, dtype)
    exact_f32(ev["dS"], "dS")
    exact_f32(ev["dot"], "dot")
    dSo, Po = rt(ev["dS"]), rt(ev["P"])
    representable(ev["P"], BF16)
    step = 2.0 ** -12
    check_sum(dSo.abs(), k.abs(), step)
    check_sum(dSo.abs().transpose(2, 3), q.abs(), step * 2.0 ** -10)
    check_sum(Po.transpose(2, 3), ac["dO"].abs(), 1.0 / 64)
    check_accumulation(1, (float(ev["dS"].abs().sum(0).max()) / step,))
    dq_s = scaled_f32(exact_f32(merge_heads(ev["dq"]), "dq"), S.QSCALE_PLAIN32).double()
    dqkv = rt(torch.cat([dq_s, exact_f32(merge_heads(ev["dk"]), "dk"), exact_f32(merge_heads(ev["dvt"].transpose(2, 3)), "dv")], 1))
    if kind == "onehot":
        assert not bool(ev["dS"].any()) and not bool(dqkv[:, :2 * C].any())
    else:                                                                          # "uniform", and the rows of "table" whose table entry points outside the window
        assert bool(dqkv[:, :C].any()) and not bool(dqkv[:, C:2 * C].any())
    assert bool(dqkv[:, 2 * C:].any())
    gwqkv, gbqkv = dqkv.t() @ xn, dqkv.sum(0)
    bounds = {}
    if kind != "onehot":
        bw = torch.zeros(3 * C, C, dtype=torch.float64)
        bw[:C] = (M - 1) * 2.0 ** -24 * (dqkv[:, :C].abs().t() @ xn.abs())
        bb = torch.zeros(3 * C, dtype=torch.float64)
        bb[:C] = (M - 1) * 2.0 ** -24 * dqkv[:, :C].abs().sum(0)
        bounds = {"wqkv": bw, "bqkv": bb}
    check_sum(dqkv[:, C:].abs().t(), xn.abs(), 1.0 / 64)
    check_accumulation(1, (float(dqkv[:, C:].abs().sum(0).max()) * 64,))
    dxn = rt(exact_f32(dqkv @ wqkv, "dxn"))
    check_sum(dqkv.abs(), wqkv.abs(), 2.0 ** -16)
    gmod = None
    if c["mod"] is not None:
        gmod = exact_f32(dxn.reshape(n, 64, C).sum(0), "modulator gradient")
        check_accumulation(1, (float(dxn.abs().reshape(n, 64, C).sum(0).max()) * 64,))
    # LN1 backward on dxn (window order) plus the residual path dx1
    gamma1 = c["gamma1"]
    xr = x[tok]
    xhat, rstd = xr / a[tok], 1.0 / a[tok]
    g_ = dxn * gamma1
    s1, s2 = exact_f32(g_.sum(1, keepdim=True), "sum g") / C, exact_f32((g_ * xhat).sum(1, keepdim=True), "sum g xhat") / C
    check_accumulation(1, (float(g_.abs().sum(1).max()) * 64,))
    t2 = exact_f32(exact_f32(g_ - s1, "g - s1") - xhat * s2, "g - s1 - xhat s2")
    exact_f32(g_ - xhat * s2, "g - xhat s2")
    r = exact_f32(exact_f32(t2 * rstd, "dx of LN1") + dx1[tok], "dx")
    dx = torch.zeros(M, C, dtype=torch.float64)
    dx[tok] = r
    gn1w, gn1b = exact_f32((dxn * xhat).sum(0), "norm1_w"), exact_f32(dxn.sum(0), "norm1_b")
    check_accumulation(1, (float(dxn.abs().sum(0).max()) * 64,))
    dtable = rpb_table_grad64(ev["dbias"])
    refs = {"dx": dx, "norm1_w": gn1w, "norm1_b": gn1b, "rpb_table": dtable, "wqkv": gwqkv, "bqkv": gbqkv, "wproj": gwp, "bproj": gbp}
    if gmod is not None:
        refs["modulator"] = gmod
    for key, val in refs.items():
        if key == "rpb_table" and kind == "onehot":
            assert not bool(val.any())
        else:
            assert bool(val.any()), f"{key} is identically zero"
    if dtype != F32:
        assert not torch.equal(dx, dx1), "dxn must reach dx through LayerNorm 1"
    return {"x": x, "dx1": dx1, "drop": drop if dropped else None, "sd": S.block_state_dict(c, C), "heads": heads, "refs": refs, "bounds": bounds, "dxn": dxn, "tok": tok,
            "mod": c["mod"], "n": n}


def modulator_grad_wrong_axis(c, C):
    """fault stand-in: the modulator gradient summed over the 64 window positions (and spread over them) instead of over the windows"""
    d = c["dxn"].reshape(c["n"], 64, C)
    return d.sum(1, keepdim=True).expand(c["n"], 64, C).sum(0) / 64 * c["n"]
