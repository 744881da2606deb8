"""Exact cases of the cross-modulator attention kernel (uf_cross_attn_fwd) on saturated lattices (helpers; no GPU needed), in the manner of
tests/saturated_lattice.py, whose building blocks this file imports.

The kernel is x += proj(softmax(q K_h^T) V_h) with q = T((T(x) Wq^T + bq) hd^-0.5) for every row on its own against 64 shared keys.  Two kinds
of input make it a linear map on small integers:

  "onehot"   the channels of a row are, per head, a signed Hadamard code times an amplitude of 1 or 2, and Wq = 32 I, bq = 0.  Rounding is symmetric,
             so q_h = r * code with ONE T value r per (row, head) whatever the head width (hd^-0.5 is a power of two only at hd 16), and the logits
             are r (code . key).  The keys are signed codes times amplitudes 1 / 2 / 4: the key that holds the query's code scores r hd amp, its
             negative -r hd amp, every other key 0 (Hadamard rows are orthogonal).  Head width 32 has 64 distinct signed codes; head width 16 has 32,
             so every code is held by two keys whose amplitudes differ by a factor of two -- the larger wins.  The winner leads by at least 160 in
             the log2 domain (``LEAD2``, asserted on the reference logits): e is 1 for it and exactly 0 for the rest in float32, the sum is 1, and o
             is the winner's V row.
  "uniform"  Wq = 0 and bq = 0: every logit is 0, e = 1 for all 64 keys, the sum is 64 and o is the mean of V over the keys, a multiple of 1/64.

V is odd (1 or 3 times one sign per head and channel), Wp has three entries of +-1 per row, bp and (uniform) x are small integers: the float32
projection and the residual are exact.  Every condition is asserted on the float64 reference alone, by ``cross_case``; the gate is
exact_lattice.assert_exact on every element."""
import functools

import torch

import saturated_lattice as SL
from exact_lattice import F32, BF16, F16, PM2, check_accumulation, check_representable, lattice

MODES = [F32, BF16, F16]
KINDS = ("onehot", "uniform")
# (M, C, heads): head widths 16 and 32; C = 16, 32, 64, 256 and 512; M = 128 is two 64-row tiles (four 32-row tiles for f32 at C = 512)
CASES = [(128, 16, 1), (128, 32, 1), (128, 32, 2), (128, 64, 2), (128, 64, 4), (128, 256, 8), (128, 512, 32)]
Q_GAIN = 32.0
LEAD2 = 160.0                    # asserted lead in the log2 domain: 150 (2^-150 is below half the smallest float32 subnormal) + slack for the rounding of q
LOG2E = 1.4426950408889634


def cross_doc64(x, wq, bq, k, vt, wp, bp, dtype):
    """The documented formula (include/uformer_hip.h) in float64 with its rounding points: x rounded to T as the GEMM operand; q = (x Wq^T + bq)
    times float32(hd^-0.5) in float32, rounded to T; e = exp(s - max) rounded to T as the operand of e V; o = (e V) / sum(e) rounded to T; the
    projection, the bias and the residual unrounded.  x (M, C), k (heads, 64, hd), vt (heads, hd, 64) float64 ->
    dict(q (heads, M, hd), s logits (heads, M, 64), e as T, esum, o (M, C) before its rounding, out (M, C))."""
    heads, _, hd = k.shape
    M, C = x.shape
    xt = x.to(dtype).double()
    acc = (xt @ wq.t() + bq).float()
    assert torch.equal(acc.double(), xt @ wq.t() + bq), "the q accumulator is not a float32 value"
    q = (acc * torch.tensor(hd ** -0.5, dtype=torch.float32)).to(dtype).double().reshape(M, heads, hd).transpose(0, 1)
    s = q @ k.transpose(1, 2)
    e = torch.exp(s - s.max(2, keepdim=True).values)
    eT = e.to(dtype)
    o = ((eT.double() @ vt.transpose(1, 2)) / e.sum(2, keepdim=True)).transpose(0, 1).reshape(M, C)
    out = x + o.to(dtype).double() @ wp.t() + bp
    return {"q": q, "s": s, "e": eT, "esum": e.sum(2), "o": o, "out": out}


def key_codes(hd, g):
    """(code index, amplitude) of the 64 keys of one head.  hd 32: the 64 signed codes once each, amplitudes 1 / 2 / 4.  hd 16: the 32 signed codes
    twice each, the two holders of a code at amplitudes (a, 2a), a = 1 or 2 -- the tie is broken by amplitude."""
    if hd == 32:
        return torch.randperm(64, generator=g), torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (64,), generator=g)]
    base = torch.tensor((1.0, 2.0), dtype=torch.float64)[torch.randint(2, (32,), generator=g)]
    code = torch.arange(32).repeat(2)
    amp = torch.cat([base, 2 * base])
    p = torch.randperm(64, generator=g)
    return code[p], amp[p]


@functools.lru_cache(maxsize=None)
def cross_case(kind, M, C, heads, dtype):
    assert kind in KINDS and C % heads == 0 and M % 64 == 0
    hd = C // heads
    assert hd in (16, 32)
    g = SL.gen(700 + C + heads)
    codes = SL.signed_codes(hd)                                              # (2 hd, hd)
    k = torch.zeros(heads, 64, hd, dtype=torch.float64)
    x = torch.zeros(M, C, dtype=torch.float64)
    target = torch.zeros(heads, M, dtype=torch.long)                         # the key each query must select
    for h in range(heads):
        kc, ka = key_codes(hd, g)
        k[h] = codes[kc] * ka[:, None]
        want = torch.randint(64, (M,), generator=g)                          # the query holds this key's code ...
        ax = torch.tensor((1.0, 2.0), dtype=torch.float64)[torch.randint(2, (M,), generator=g)]
        x[:, h * hd:(h + 1) * hd] = codes[kc[want]] * ax[:, None]
        same = kc[None, :] == kc[want][:, None]                              # ... and the winner is its holder of the largest amplitude
        target[h] = torch.where(same, ka[None, :], torch.zeros(1, dtype=torch.float64)).argmax(1)
    vt = SL.pick(SL.V_VALUES, (heads, hd, 64), 710 + C + heads) * SL.pick((-1, 1), (heads, hd, 1), 711 + C + heads)
    wp, bp = SL.sparse_pm1(C, C, 720 + C), lattice((C,), PM2, 721 + C)
    bq = torch.zeros(C, dtype=torch.float64)
    if kind == "onehot":
        wq = Q_GAIN * torch.eye(C, dtype=torch.float64)
    else:
        wq = torch.zeros(C, C, dtype=torch.float64)
        x = lattice((M, C), PM2, 730 + C)
    check_representable(x, dtype)
    check_representable(k, dtype)
    check_representable(vt, dtype)
    d = cross_doc64(x, wq, bq, k, vt, wp, bp, dtype)
    # conditions, on the reference alone
    s, e64 = d["s"], d["e"].double()
    top = s.max(2, keepdim=True).values
    winners = s == top
    n_win = winners.sum(2)
    if kind == "onehot":
        rest = torch.where(winners, torch.full_like(s, -1e9), s).max(2).values
        lead2 = (top[..., 0] - rest) * LOG2E
        assert float(lead2.min()) >= LEAD2, f"a non-winner within {float(lead2.min())} of the winner in the log2 domain"
        assert float(lead2.min()) / LOG2E >= SL.MARGIN                      # f32 takes exp, not exp2: 104 in the natural domain
        assert bool((n_win == 1).all()) and bool(winners.gather(2, target[..., None]).all()), "the selected key is not the only winner"
        assert len(target.unique()) >= (24 if hd == 16 else 40)              # the queries select many different keys (hd 16: 32 can win)
        q = d["q"]
        assert bool((q.abs() == q.abs()[..., :1]).all()) and float(q.abs().min()) >= 4      # q_h = r * code with one T value r per (row, head)
        lead = float(lead2.min())
    else:
        assert bool((n_win == 64).all()) and bool((s == 0).all())
        lead = 0.0
    assert bool(((e64 == 1.0) | (e64 == 0.0)).all()) and bool((e64[winners] == 1.0).all())
    assert torch.equal(d["esum"].float().double(), n_win.double()), "the float32 sum is not the number of winners"
    exact_o = (winners.double() @ vt.transpose(1, 2) / n_win[..., None]).transpose(0, 1).reshape(M, C)
    assert torch.equal(d["o"].to(dtype).double(), exact_o), "the documented softmax does not round to the lattice value"
    check_representable(exact_o, dtype, step=1.0 / 64)
    assert bool((exact_o != 0).all())
    check_accumulation(hd, (int(d["q"].abs().max()) + 1,), (4,))
    check_accumulation(3, (3 * 64,), (1,), addend_steps=(2 + 2) * 64)       # the projection in steps of 1/64, + bias + residual
    out = x + exact_o @ wp.t() + bp
    assert torch.equal(d["out"], out) and torch.equal(out.float().double(), out)
    return {"x": x, "wq": wq, "bq": bq, "k": k, "vt": vt, "wp": wp, "bp": bp, "o": exact_o, "out": out, "target": target, "lead2": lead, "n_win": n_win}


def faulty_out(c, dtype, **fault):
    """the reference of ``cross_case`` again under one fault (stand-ins of the CPU twin): ``v_rowmajor``: v^T read as if it were v; ``head_roll``: the
    keys of the next head; ``no_residual``: the branch alone"""
    x, k, vt = c["x"], c["k"], c["vt"]
    heads, _, hd = k.shape
    if fault.get("v_rowmajor"):
        vt = vt.reshape(heads, 64, hd).transpose(1, 2)
    if fault.get("head_roll"):
        k = k.roll(1, 0)
    M, C = x.shape
    q = ((x.to(dtype).double() @ c["wq"].t() + c["bq"]).float() * torch.tensor(hd ** -0.5, dtype=torch.float32)).to(dtype).double()
    s = q.reshape(M, heads, hd).transpose(0, 1) @ k.transpose(1, 2)
    e = torch.exp(s - s.max(2, keepdim=True).values)
    o = ((e.to(dtype).double() @ vt.transpose(1, 2)) / e.sum(2, keepdim=True)).transpose(0, 1).reshape(M, C).to(dtype).double()
    return (0.0 if fault.get("no_residual") else x) + o @ c["wp"].t() + c["bp"]
