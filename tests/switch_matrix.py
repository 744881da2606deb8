"""The model switches taken together: which combinations build, the committed case lists that cover them, ONE float64 reference
for all of them, the stand-in faults that measure the gates' strength, and the comparison functions the CPU and the GPU file share.

* ``buildable(form)``: a pure predicate over the architecture factors, written from DESIGN.md / uformer_amd/spec.py; it never calls a constructor
  (tests/test_switch_matrix_reference.py holds it against ``model.Uformer`` over the full product).
* ``INFER_ROWS`` / ``TRAIN_ROWS``: literal lists of row names.  A name spells its levels (``e16-128x256-ffn-conv-x-d6c3-nomod-mask-B3-f16-graph``);
  ``parse_infer`` / ``parse_train`` read them back.  ``generate_infer_rows`` / ``generate_train_rows`` are the deterministic generators that wrote
  the lists: every architecture form, then rows until every legal pair of levels of any two factors is covered.
* ``reference_forward`` / ``reference_grads``: the per-block compositions of tests/crossmod_composition.py (which dispatches to the ffn / conv /
  rectangular ones) for 8x8-window blocks and ``block4`` for the 4x4-window bottleneck of an img-64 form, in float64; gradients are torch autograd
  through it under ``O.charbonnier_loss``.  ``fault=`` applies one stand-in wiring fault to the REFERENCE.
* ``output_gate`` / ``grad_rel``: the whole-model gates of tests/test_gpu_model.py and tests/test_gpu_bwd.py.  No tolerance of this file's own.

Plain torch / numpy, CPU only, no library load.  TEST INFRASTRUCTURE ONLY."""
import contextlib
import dataclasses
import itertools
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

import crossmod_composition as XC
import rect_composition as RC
from oracle import uformer_oracle as O
from uformer_amd import spec

Tensor = torch.Tensor

# ---- gates: copied, with their sources -----------------------------------------------------------------------------------------------------------
F32_TOL, BF16_TOL, BF16_PSNR = 1e-3, 4e-3, 60.0                                               # tests/test_gpu_model.py
GRAD_RTOL = {torch.float32: 2e-3, torch.bfloat16: 6e-2, torch.float16: 1e-2}                  # tests/test_gpu_bwd.py (2e-3, GRAD_RTOL_BF16, GRAD_RTOL_F16)
F16_LOSS_SCALE = 65536.0                                                                      # tests/test_gpu_bwd.py
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HEADS = (1, 2, 4, 8, 16, 16, 8, 4, 2)
DEPTHS = {16: (1,) * 9, 32: (1, 2, 2, 2, 2, 2, 2, 2, 1), 64: (1,) * 9}                         # tiny32's depths at 32: the only width whose stages shift


def output_gate(y: Tensor, ref: Tensor, dtype) -> Tuple[bool, float, float]:
    """(passes, max-abs error, PSNR): f32 and f16 max-abs <= F32_TOL; bf16 max-abs <= BF16_TOL and PSNR >= BF16_PSNR."""
    y, ref = y.detach().float().cpu(), ref.detach().float().cpu()
    if y.shape != ref.shape or not bool(torch.isfinite(y).all()):
        return False, float("inf"), 0.0
    err = (y - ref).abs().max().item()
    ps = O.psnr(y, ref)
    if dtype in (torch.float32, torch.float16):
        return err <= F32_TOL, err, ps
    return err <= BF16_TOL and ps >= BF16_PSNR, err, ps


def grad_rel(g: Tensor, g_ref: Tensor) -> float:
    """max |g - g_ref| / max |g_ref| over the full tensor (tests/test_gpu_bwd.py's element gate); compare with GRAD_RTOL[dtype]."""
    g, g_ref = g.detach().double().cpu(), g_ref.detach().double().cpu()
    if g.shape != g_ref.shape or not bool(torch.isfinite(g).all()):
        return float("inf")
    return (g - g_ref).abs().max().item() / max(g_ref.abs().max().item(), 1e-30)


# ---- factors -------------------------------------------------------------------------------------------------------------------------------------
ARCH_FACTORS = {
    "e": (16, 32, 64),
    "img": (128, 64),
    "mlp": ("leff", "ffn"),
    "proj": ("lin", "conv"),
    "cross": ("nox", "x"),
    "chans": ("d3c3", "d6c3", "d1c1", "d4c4"),
    "mod": ("mod", "nomod"),
}
GEOMETRIES = {128: ("128x128", "128x256", "256x128"), 64: ("64x64", "64x192", "128x64")}
SHAPES = ("sq", "wide", "tall")                                # index into GEOMETRIES[img]
RUN_FACTORS = {
    "geom": GEOMETRIES[128] + GEOMETRIES[64],           # six levels; each belongs to one img_size
    "mask": ("nomask", "mask"),
    "B": (1, 3, 8),
    "dt": ("bf16", "f16"),
    "ex": ("eager", "graph", "pipe"),
}
TRAIN_RUN_FACTORS = {"geom": SHAPES, "B": (1, 2, 3), "dt": ("bf16", "f16")}
SWITCHES = ("mlp", "proj", "cross")
PROJ = {"lin": "linear", "conv": "conv"}


@dataclasses.dataclass(frozen=True)
class Form:
    """one construction: the architecture factors"""
    e: int
    img: int
    mlp: str = "leff"
    proj: str = "lin"
    cross: str = "nox"
    chans: str = "d3c3"
    mod: str = "mod"

    @property
    def dd_in(self) -> int:
        return int(self.chans[1])

    @property
    def in_chans(self) -> int:
        return int(self.chans[3])

    def arch(self) -> Tuple:
        return (self.e, self.img, self.mlp, self.proj, self.cross)

    def cfg(self) -> spec.UformerConfig:
        return spec.UformerConfig(img_size=self.img, in_chans=self.in_chans, dd_in=self.dd_in, embed_dim=self.e, depths=DEPTHS[self.e], num_heads=HEADS,
                                  modulator=self.mod == "mod", token_mlp=self.mlp, token_projection=PROJ[self.proj], cross_modulator=self.cross == "x")

    def ctor_kwargs(self) -> dict:
        c = self.cfg()
        return dict(img_size=c.img_size, in_chans=c.in_chans, dd_in=c.dd_in, embed_dim=c.embed_dim, depths=list(c.depths), num_heads=list(c.num_heads),
                    modulator=c.modulator, token_mlp=c.token_mlp, token_projection=c.token_projection, cross_modulator=c.cross_modulator)


def all_forms() -> List[Form]:
    return [Form(*lv) for lv in itertools.product(*ARCH_FACTORS.values())]


def buildable(form: Form) -> Optional[str]:
    """None if ``model.Uformer(**form.ctor_kwargs())`` builds, else the name of the option that the constructor refuses.
    The three switches need every block on 8x8 windows (img_size 64 clamps the bottleneck to 4x4) and every block width <= 512 with head_dim 16 or
    32 for 'ffn' and the cross-modulator, <= 512 for 'conv' (embed_dim 64 has a 1024-wide bottleneck).  embed_dim 64 at img_size 64 would run
    the 4x4-window bottleneck at head_dim 64, which uf_win4.hip does not build: this matrix found that form building and failing at its first
    forward, and the constructor refuses it since."""
    if form.dd_in == 3 and form.in_chans != 3:
        return "in_chans"
    if not 1 <= form.dd_in <= spec.MAX_DD_IN:
        return "dd_in"
    if not 1 <= form.in_chans <= spec.MAX_IN_CHANS:
        return "in_chans"
    if form.img not in (64, 128) and form.img % 128:
        return "img_size"
    if form.img == 64 and form.e == 64:                 # the 4x4-window kernels are built for head_dim 16 and 32
        return "embed_dim"
    for name, off, label in (("cross", "nox", "cross_modulator"), ("proj", "lin", "token_projection"), ("mlp", "leff", "token_mlp")):
        if getattr(form, name) != off and (form.img == 64 or form.e == 64):
            return label
    return None


def trainable(form: Form) -> Optional[str]:
    """None if the form trains: token_projection='linear' without the cross-modulator."""
    why = buildable(form)
    if why:
        return why
    if form.proj != "lin":
        return "token_projection"
    if form.cross != "nox":
        return "cross_modulator"
    return None


ARCH_FORMS = sorted({f.arch() for f in all_forms() if buildable(f) is None}, key=lambda a: (a[1] != 128, a[0], a[2], a[3], a[4]))       # the 19
TRAIN_FORMS = [a for a in ARCH_FORMS if a[3] == "lin" and a[4] == "nox"]                                                               # the 7


# ---- rows ----------------------------------------------------------------------------------------------------------------------------------------
INFER_KEYS = tuple(ARCH_FACTORS) + tuple(RUN_FACTORS)
TRAIN_KEYS = tuple(ARCH_FACTORS) + tuple(TRAIN_RUN_FACTORS) + ("ckpt",)
INFER_LEVELS = {**ARCH_FACTORS, **RUN_FACTORS}
TRAIN_REMAINING = ("chans", "mod", "geom", "B", "dt")
TRAIN_LEVELS = {**ARCH_FACTORS, **TRAIN_RUN_FACTORS}                   # 'ckpt' is not searched: every configuration is emitted with both values


def pair_legal(k1, v1, k2, v2) -> bool:
    """May level v1 of factor k1 and level v2 of factor k2 stand in one row?  Every rule of the matrix is a rule between two levels:
    a switch that is on needs img 128 and embed_dim <= 32; a user mask needs img 128 (4x4-window blocks take none) and the eager execution
    (GraphedForward and PipelinedForward take the image alone)."""
    d = {k1: v1, k2: v2}
    if d.get("geom") not in (None,) + SHAPES:
        img = 128 if d["geom"] in GEOMETRIES[128] else 64
        if d.setdefault("img", img) != img:
            return False
    on = [k for k in SWITCHES if k in d and d[k] != ARCH_FACTORS[k][0]]
    if on and (d.get("img") == 64 or d.get("e") == 64):
        return False
    if d.get("img") == 64 and d.get("e") == 64:
        return False
    if d.get("mask") == "mask" and (d.get("img") == 64 or d.get("ex", "eager") != "eager"):
        return False
    return True


def row_legal(row: Dict) -> bool:
    return all(pair_legal(a, row[a], b, row[b]) for a, b in itertools.combinations(row, 2))


def legal_pairs(levels: Dict) -> set:
    return {(a, va, b, vb) for a, b in itertools.combinations(levels, 2) for va in levels[a] for vb in levels[b] if pair_legal(a, va, b, vb)}


def row_pairs(row: Dict, keys) -> set:
    return {(a, row[a], b, row[b]) for a, b in itertools.combinations(keys, 2)}


def _complete(row: Dict, levels: Dict, todo: set) -> Dict:
    """fill the factors ``row`` leaves open, one at a time in the order of ``levels``, each with the legal level that covers most pairs of
    ``todo`` against the factors already set (ties: the level used least so far comes first -- the caller rotates ``levels``)"""
    row = dict(row)
    for k in levels:
        if k in row:
            continue
        best, best_n = None, -1
        for v in levels[k]:
            if not all(pair_legal(k, v, a, row[a]) for a in row):
                continue
            n = sum(((a, row[a], k, v) in todo) or ((k, v, a, row[a]) in todo) for a in row)
            if n > best_n:
                best, best_n = v, n
        assert best is not None, (row, k)
        row[k] = best
    return {k: row[k] for k in levels}


def _generate(levels: Dict, seeds: List[Dict], among=None) -> List[Dict]:
    """``seeds`` completed one by one, then rows until every legal pair (between factors of ``among``, default all) is covered"""
    todo = {t for t in legal_pairs(levels) if among is None or (t[0] in among and t[2] in among)}
    rows = []
    rot = 0

    def rotated():
        return {k: tuple(v[(i + rot) % len(v)] for i in range(len(v))) for k, v in levels.items()}

    for s in seeds:
        row = _complete(s, {k: rotated()[k] for k in levels}, todo)
        assert row_legal(row)
        rows.append(row)
        todo -= row_pairs(row, tuple(levels))
        rot += 1
    while todo:
        a, va, b, vb = min(todo, key=lambda t: tuple(map(str, t)))
        row = _complete({a: va, b: vb}, {k: rotated()[k] for k in levels}, todo)
        assert row_legal(row)
        rows.append(row)
        todo -= row_pairs(row, tuple(levels))
        rot += 1
    return rows


def _arch_seed(a) -> Dict:
    return dict(e=a[0], img=a[1], mlp=a[2], proj=a[3], cross=a[4])


def infer_name(r: Dict) -> str:
    return "-".join([f"e{r['e']}", r["geom"], r["mlp"], r["proj"], r["cross"], r["chans"], r["mod"],
                     r["mask"], f"B{r['B']}", r["dt"], r["ex"]])


def train_name(r: Dict) -> str:
    return "-".join([f"e{r['e']}", GEOMETRIES[r["img"]][SHAPES.index(r["geom"])], r["mlp"], r["proj"], r["cross"], r["chans"], r["mod"],
                     f"B{r['B']}", r["dt"], r["ckpt"]])


def _parse_common(tok: List[str]) -> Dict:
    img, gi = next((i, g.index(tok[1])) for i, g in GEOMETRIES.items() if tok[1] in g)
    return dict(e=int(tok[0][1:]), img=img, mlp=tok[2], proj=tok[3], cross=tok[4], chans=tok[5], mod=tok[6], geom=tok[1], shape=SHAPES[gi])


def parse_infer(name: str) -> Dict:
    tok = name.split("-")
    r = _parse_common(tok)
    r.update(mask=tok[7], B=int(tok[8][1:]), dt=tok[9], ex=tok[10])
    return {k: r[k] for k in INFER_KEYS}


def parse_train(name: str) -> Dict:
    tok = name.split("-")
    r = _parse_common(tok)
    r.update(B=int(tok[7][1:]), dt=tok[8], ckpt=tok[9], geom=r["shape"])
    return {k: r[k] for k in TRAIN_KEYS}


def generate_infer_rows() -> List[str]:
    return [infer_name(r) for r in _generate(INFER_LEVELS, [_arch_seed(a) for a in ARCH_FORMS])]


def generate_train_rows() -> List[str]:
    """every trainable architecture form, then configurations until every pair of levels of the remaining factors (channel counts, modulator,
    shape of the input, batch, 2-byte type) is covered; each configuration with use_checkpoint off ('kept') and on ('ckpt'), same input and seed"""
    levels = {k: v for k, v in TRAIN_LEVELS.items()}
    levels.update(proj=("lin",), cross=("nox",))
    out = []
    for r in _generate(levels, [_arch_seed(a) for a in TRAIN_FORMS], among=TRAIN_REMAINING):
        out += [train_name({**r, "ckpt": c}) for c in ("kept", "ckpt")]
    return out


def form_of(row: Dict) -> Form:
    return Form(**{k: row[k] for k in ARCH_FACTORS})


def geometry(row: Dict) -> Tuple[int, int]:
    g = row["geom"]
    h, w = (GEOMETRIES[row["img"]][SHAPES.index(g)] if g in SHAPES else g).split("x")
    return int(h), int(w)


# written by ``python tests/switch_matrix.py``; tests/test_switch_matrix_reference.py holds them equal to the generators' output
INFER_ROWS: List[str] = [
    "e16-128x128-ffn-conv-nox-d3c3-mod-nomask-B1-bf16-eager",
    "e16-128x256-ffn-conv-x-d6c3-nomod-mask-B3-f16-eager",
    "e16-256x128-ffn-lin-nox-d1c1-nomod-nomask-B8-f16-pipe",
    "e16-128x128-ffn-lin-x-d4c4-mod-mask-B8-bf16-eager",
    "e16-128x256-leff-conv-nox-d4c4-nomod-nomask-B3-bf16-graph",
    "e16-256x128-leff-conv-x-d1c1-mod-mask-B1-f16-eager",
    "e16-128x128-leff-lin-nox-d6c3-mod-nomask-B3-bf16-pipe",
    "e16-128x256-leff-lin-x-d3c3-nomod-mask-B8-f16-eager",
    "e32-256x128-ffn-conv-nox-d3c3-mod-mask-B3-bf16-eager",
    "e32-128x128-ffn-conv-x-d6c3-nomod-nomask-B1-f16-graph",
    "e32-128x256-ffn-lin-nox-d1c1-mod-nomask-B1-bf16-graph",
    "e32-256x128-ffn-lin-x-d4c4-nomod-mask-B8-f16-eager",
    "e32-128x128-leff-conv-nox-d3c3-mod-nomask-B8-bf16-pipe",
    "e32-256x128-leff-conv-x-d6c3-nomod-mask-B8-f16-eager",
    "e32-128x128-leff-lin-nox-d1c1-mod-nomask-B3-bf16-pipe",
    "e32-128x128-leff-lin-x-d4c4-nomod-mask-B1-f16-eager",
    "e64-128x128-leff-lin-nox-d3c3-mod-nomask-B3-bf16-graph",
    "e16-128x64-leff-lin-nox-d6c3-nomod-nomask-B8-f16-graph",
    "e32-64x64-leff-lin-nox-d1c1-mod-nomask-B1-bf16-pipe",
    "e32-128x64-leff-lin-nox-d1c1-mod-nomask-B3-bf16-eager",
    "e16-64x192-leff-lin-nox-d1c1-mod-nomask-B8-bf16-pipe",
    "e16-128x64-leff-lin-nox-d3c3-nomod-nomask-B1-f16-pipe",
    "e32-64x192-leff-lin-nox-d3c3-nomod-nomask-B3-f16-graph",
    "e16-64x64-leff-lin-nox-d3c3-nomod-nomask-B8-f16-eager",
    "e64-128x256-leff-lin-nox-d4c4-nomod-nomask-B1-f16-pipe",
    "e32-128x64-leff-lin-nox-d4c4-nomod-nomask-B3-f16-graph",
    "e16-64x192-leff-lin-nox-d4c4-mod-nomask-B1-bf16-eager",
    "e16-64x64-leff-lin-nox-d4c4-nomod-nomask-B3-f16-graph",
    "e32-64x192-leff-lin-nox-d6c3-mod-nomask-B3-bf16-graph",
    "e16-64x64-leff-lin-nox-d6c3-nomod-nomask-B8-f16-pipe",
    "e16-128x128-leff-lin-x-d1c1-mod-nomask-B1-bf16-pipe",
    "e64-256x128-leff-lin-nox-d6c3-nomod-mask-B8-f16-eager",
    "e64-256x128-leff-lin-nox-d1c1-mod-nomask-B8-bf16-graph",
]
TRAIN_ROWS: List[str] = [
    "e16-128x128-ffn-lin-nox-d3c3-mod-B1-bf16-kept",
    "e16-128x128-ffn-lin-nox-d3c3-mod-B1-bf16-ckpt",
    "e16-128x256-leff-lin-nox-d6c3-nomod-B2-f16-kept",
    "e16-128x256-leff-lin-nox-d6c3-nomod-B2-f16-ckpt",
    "e32-256x128-ffn-lin-nox-d1c1-mod-B3-f16-kept",
    "e32-256x128-ffn-lin-nox-d1c1-mod-B3-f16-ckpt",
    "e32-128x128-leff-lin-nox-d4c4-nomod-B3-bf16-kept",
    "e32-128x128-leff-lin-nox-d4c4-nomod-B3-bf16-ckpt",
    "e64-256x128-leff-lin-nox-d3c3-nomod-B2-bf16-kept",
    "e64-256x128-leff-lin-nox-d3c3-nomod-B2-bf16-ckpt",
    "e16-128x64-leff-lin-nox-d6c3-mod-B1-f16-kept",
    "e16-128x64-leff-lin-nox-d6c3-mod-B1-f16-ckpt",
    "e32-64x64-leff-lin-nox-d1c1-nomod-B1-bf16-kept",
    "e32-64x64-leff-lin-nox-d1c1-nomod-B1-bf16-ckpt",
    "e32-64x192-leff-lin-nox-d1c1-mod-B2-bf16-kept",
    "e32-64x192-leff-lin-nox-d1c1-mod-B2-bf16-ckpt",
    "e64-128x256-leff-lin-nox-d3c3-mod-B3-f16-kept",
    "e64-128x256-leff-lin-nox-d3c3-mod-B3-f16-ckpt",
    "e16-64x192-leff-lin-nox-d4c4-mod-B1-f16-kept",
    "e16-64x192-leff-lin-nox-d4c4-mod-B1-f16-ckpt",
    "e32-256x128-leff-lin-nox-d4c4-mod-B2-bf16-kept",
    "e32-256x128-leff-lin-nox-d4c4-mod-B2-bf16-ckpt",
    "e64-128x128-leff-lin-nox-d6c3-nomod-B3-f16-kept",
    "e64-128x128-leff-lin-nox-d6c3-nomod-B3-f16-ckpt",
    "e16-128x128-leff-lin-nox-d6c3-mod-B2-bf16-kept",
    "e16-128x128-leff-lin-nox-d6c3-mod-B2-bf16-ckpt",
]
# Rows replaced by the same levels at another seed: at the default seed the reference with parameters rounded to the row's 2-byte type left more than
# half that type's gate -- for bf16 both parts of it, max-abs and PSNR (tests/test_switch_matrix_reference.py; keyed by the name without -kept / -ckpt).
SEED_OVERRIDE: Dict[str, int] = {
    "e32-128x256-ffn-lin-nox-d1c1-mod-nomask-B1-bf16-graph": 6137,          # 3.46e-3 -> under 2e-3
    "e32-256x128-ffn-lin-x-d4c4-nomod-mask-B8-f16-eager": 6881,             # 5.32e-4 -> under 5e-4
    "e64-256x128-leff-lin-nox-d1c1-mod-nomask-B8-bf16-graph": 3545,         # 2.65e-3 -> 1.65e-3 (the seventh seed: the fourth, 3524, met the max-abs half
                                                                            # alone: its PSNR of 65.7 dB is under the 66.02 dB that half the rms error of 60 dB means)
}
# Rows for which eight seeds did not do it (bf16 rounding of the parameters alone moves these outputs by 2.3e-3 ... 4.3e-3, the bf16 gate being 4e-3):
# their parameters are drawn and then rounded to bf16, so that a bf16 run reads exactly the parameters of the reference and what is left on the GPU
# is the kernel path's.  The float32 run of the same row reads them too.
BF16_REPRESENTABLE_ROWS = (
    "e32-256x128-ffn-conv-nox-d3c3-mod-mask-B3-bf16-eager",                 # 2.75e-3 ... 4.30e-3 over eight seeds
    "e64-128x128-leff-lin-nox-d3c3-mod-nomask-B3-bf16-graph",               # 2.28e-3 ... 3.47e-3
    "e64-256x128-leff-lin-nox-d3c3-nomod-B2-bf16",                          # 2.11e-3 ... over eight seeds
)
# spec.synth_state_dict draws the relative-position tables at 0.2 sigma.  At that scale the bottleneck's table transposed (a stand-in fault) moves
# the output by 5e-5 ... 1.4e-3: under the f32 gate on most rows.  The rows therefore scale the bottleneck's tables (sigma 6.4: attention that follows
# position, as trained tables do); tests/test_switch_matrix_reference.py prints the margin this leaves on every row.
BOTTLENECK_RPB_SCALE = 32.0
IMAGE_PATTERN = {1: (0,), 2: (0, 1), 3: (0, 1, 0), 8: (0, 1, 1, 0, 0, 1, 0, 1)}              # a batch is made of the row's two distinct images


def row_seed(name: str) -> int:
    import zlib
    base = name.rsplit("-", 1)[0] if name.endswith(("-kept", "-ckpt")) else name         # a kept / ckpt pair shares input and seed
    return SEED_OVERRIDE.get(base, 1000 + zlib.crc32(base.encode()) % 9000)


def row_inputs(name: str, row: Dict):
    """(sd, two distinct images (2, dd_in, H, W), one mask (1, 1, H, W) shared by the batch -- the reference's mask path adds a (nW, 64, 64)
    shift mask to it, so it takes one -- or None, target images for the training loss) of a row"""
    form, seed = form_of(row), row_seed(name)
    H, W = geometry(row)
    sd = spec.synth_state_dict(form.cfg(), seed)
    for k in sd:                                  # see BOTTLENECK_RPB_SCALE
        if k.startswith("conv.") and k.endswith("relative_position_bias_table"):
            sd[k] = (sd[k] * BOTTLENECK_RPB_SCALE).to(torch.bfloat16).float()        # representable: a 2-byte run reads the same table
    base = name.rsplit("-", 1)[0] if name.endswith(("-kept", "-ckpt")) else name
    if base in BF16_REPRESENTABLE_ROWS:
        sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    x = spec.synth_input(2, H, W, seed + 1, channels=form.dd_in)
    mask = None
    if row.get("mask") == "mask":
        mask = (torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(seed + 2)) > 0.3).float()
    target = spec.synth_input(2, H, W, seed + 3, channels=form.in_chans)
    return sd, x, mask, target


def batch_of(two: Tensor, B: int) -> Tensor:
    return two[list(IMAGE_PATTERN[B])].contiguous()


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
class _DwConv9(torch.autograd.Function):
    """depthwise 3x3, zero padding 1, as nine shifted products, with the backward written the same way (autograd through nine slices of a padded
    copy allocates a zero-filled padded gradient per tap)"""

    @staticmethod
    def forward(ctx, h, w, b):
        H, W = h.shape[-2:]
        hp = F.pad(h, (1, 1, 1, 1))
        out = b.reshape(1, -1, 1, 1).expand_as(h).clone()
        for i in range(3):
            for j in range(3):
                out.addcmul_(hp[:, :, i:i + H, j:j + W], w[:, 0, i, j].reshape(1, -1, 1, 1))
        ctx.save_for_backward(hp, w)
        return out

    @staticmethod
    def backward(ctx, g):
        hp, w = ctx.saved_tensors
        H, W = g.shape[-2:]
        gp = F.pad(g, (1, 1, 1, 1))
        dh = torch.zeros_like(g)
        dw = torch.empty_like(w)
        for i in range(3):
            for j in range(3):
                dh.addcmul_(gp[:, :, 2 - i:2 - i + H, 2 - j:2 - j + W], w[:, 0, i, j].reshape(1, -1, 1, 1))     # out[y, x] reads h[y + i - 1, x + j - 1]
                dw[:, 0, i, j] = (hp[:, :, i:i + H, j:j + W] * g).sum((0, 2, 3))
        return dh, dw, g.sum((0, 2, 3))


def dwconv9(h: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """F.conv2d(h, w, b, padding=1, groups=C) for a (C, 1, 3, 3) kernel, written as nine shifted products: float64 autograd through the grouped
    convolution is what makes the wide models slow (tests/test_switch_matrix_reference.py pins values and gradients to F.conv2d's)."""
    return _DwConv9.apply(h, w, b)


class _Gelu(torch.autograd.Function):
    """O.gelu_erf with its derivative in closed form, 0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi): one saved tensor and three
    passes where autograd through the composite keeps four and makes nine"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return O.gelu_erf(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * (0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327)


def leff9(x: Tensor, p: Dict[str, Tensor], prefix: str, H: int, W: int) -> Tensor:
    """rect_composition.leff with the depthwise convolution as nine shifted products"""
    B, L, C = x.shape
    h = _Gelu.apply(x @ p[prefix + "linear1.0.weight"].t() + p[prefix + "linear1.0.bias"])
    hid = h.shape[-1]
    h = _Gelu.apply(dwconv9(h.reshape(B, H, W, hid).permute(0, 3, 1, 2), p[prefix + "dwconv.0.weight"], p[prefix + "dwconv.0.bias"]))
    return h.permute(0, 2, 3, 1).reshape(B, L, hid) @ p[prefix + "linear2.0.weight"].t() + p[prefix + "linear2.0.bias"]


@contextlib.contextmanager
def _patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


def block4(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, H: int, W: int) -> Tensor:
    """The 4x4-window bottleneck block of an img-64 model on an H x W map (H, W multiples of 4): no shift (the constructor clamps it to 0), no
    modulator (encoder side), no mask.  ``block4_ref`` of tests/test_gpu_win4.py from the oracle's primitives at win 4; LeFF as everywhere."""
    B, L, C = x.shape
    y = O.layer_norm(x, p[prefix + "norm1.weight"], p[prefix + "norm1.bias"]).reshape(B, H, W, C)
    yw = O.window_partition(y, 4).reshape(-1, 16, C)
    aw = O.window_attention(yw, p, prefix + "attn.", heads, None)
    x = x + O.window_reverse(aw.reshape(-1, 4, 4, C), 4, H, W).reshape(B, L, C)
    z = O.layer_norm(x, p[prefix + "norm2.weight"], p[prefix + "norm2.bias"])
    return x + RC.leff(z, p, prefix + "mlp.", H, W)


FAULTS = ("modulator_dropped", "cross_skipped", "shift_mask_off", "user_mask_ignored", "global_residual", "mlp_of_previous_block", "rpb_transposed",
          "concat_swapped")


def fault_applies(fault: str, form: Form, mask: bool) -> bool:
    """does a row of this form exercise what the fault breaks?"""
    depths = DEPTHS[form.e]
    return {"modulator_dropped": form.mod == "mod", "cross_skipped": form.cross == "x", "shift_mask_off": max(depths) > 1,
            "user_mask_ignored": mask, "global_residual": True, "mlp_of_previous_block": max(depths) > 1, "rpb_transposed": True,
            "concat_swapped": True}[fault]


def _without(p: Dict, *suffixes) -> Dict:
    return {k: v for k, v in p.items() if not k.endswith(suffixes)}


def reference_forward(form: Form, sd: Dict[str, Tensor], x: Tensor, mask: Optional[Tensor] = None, fault: Optional[str] = None, **kw) -> Tensor:
    """Uformer.forward (eval mode: DropPath off) of ``form`` for a (B, dd_in, H, W) input in float64.  ``sd``: the reference-layout state dict
    (any float type; integer buffers pass through).  ``fault``: one of FAULTS, applied at a fixed place."""
    return forward_cfg(form.cfg(), sd, x, mask, fault, **kw)


def forward_cfg(cfg: spec.UformerConfig, sd: Dict[str, Tensor], x: Tensor, mask: Optional[Tensor] = None, fault: Optional[str] = None,
                dtype=torch.float64, fast_dw: bool = True) -> Tensor:
    """``reference_forward`` for any configuration (the fixtures of other depths)"""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.to(dtype)
    mask = mask.to(dtype) if mask is not None else None
    depths, heads, wins, shifts = cfg.depths, cfg.num_heads, cfg.stage_windows(), cfg.block_shifts()
    H, W = x.shape[-2:]
    hw = [(H // d, W // d) for d in cfg.stage_res_div()]
    two = [s for s in range(9) if depths[s] > 1]

    def stage(y: Tensor, s: int) -> Tensor:
        for i in range(depths[s]):
            prefix = f"{spec.STAGES[s]}.blocks.{i}."
            pb, m, ctx = p, mask, contextlib.nullcontext()
            if fault == "modulator_dropped" and s == 6 and i == depths[s] - 1:
                pb = _without(p, prefix + "modulator.weight")
            if fault == "cross_skipped" and s == 8:
                pb = _without(p, prefix + "cross_modulator.weight")
            if fault == "shift_mask_off" and two and s == two[-1] and i == 1:
                ctx = _patched(O, "shift_attn_mask", lambda Hh, Ww, win, shift: torch.zeros(((Hh // win) * (Ww // win), win * win, win * win), dtype=dtype))
            if fault == "user_mask_ignored" and s == 7:
                m = None
            if fault == "mlp_of_previous_block" and two and s == two[0] and i == 1:
                prev = f"{spec.STAGES[s]}.blocks.0.mlp."
                pb = {k: (p[prev + k[len(prefix) + 4:]] if k.startswith(prefix + "mlp.") else v) for k, v in p.items()}
            if fault == "rpb_transposed" and s == 4 and i == 0:
                n = 2 * wins[4] - 1
                key = prefix + "attn.relative_position_bias_table"
                pb = dict(p)
                pb[key] = p[key].reshape(n, n, -1).transpose(0, 1).reshape(n * n, -1)
            with ctx:
                if wins[s] == 4:
                    y = block4(y, pb, prefix, heads[s], *hw[s])
                else:
                    y = XC.lewin_block(y, pb, prefix, heads[s], shifts[s][i], *hw[s], mask=m)
        return y

    with (_patched(RC, "leff", leff9) if fast_dw else contextlib.nullcontext()):
        y = O.input_proj(x, p)
        skips = []
        for s in range(4):
            y = stage(y, s)
            skips.append(y)
            y = RC.downsample(y, p, f"dowsample_{s}.", *hw[s])
        y = stage(y, 4)
        for k in range(4):
            halves = [RC.upsample(y, p, f"upsample_{k}.", *hw[4 + k]), skips[3 - k]]
            if fault == "concat_swapped" and k == 2:
                halves.reverse()
            y = stage(torch.cat(halves, -1), 5 + k)
        y = F.conv2d(RC._tokens_to_nchw(y, H, W), p["output_proj.proj.0.weight"], p["output_proj.proj.0.bias"], stride=1, padding=1)
    residual = cfg.dd_in == 3
    if fault == "global_residual":
        residual = not residual
    return x[:, :cfg.in_chans] + y if residual else y


def reference_grads(form: Form, sd: Dict[str, Tensor], x: Tensor, target: Tensor):
    """(y, loss, dx, {parameter name: gradient}) by torch autograd through ``reference_forward`` under ``O.charbonnier_loss``, float64;
    the gradients are keyed like the reference's ``named_parameters()`` (every floating-point entry of the state dict).
    Images of the batch are independent in eval mode, so an (image, target) pair that occurs n times is run once and counted n times in the loss."""
    B = x.shape[0]
    first, count = [], []
    where = []
    for i in range(B):
        for k, j in enumerate(first):
            if torch.equal(x[i], x[j]) and torch.equal(target[i], target[j]):
                count[k] += 1
                where.append(k)
                break
        else:
            where.append(len(first))
            first.append(i)
            count.append(1)
    p = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    xr = x[first].double().clone().requires_grad_(True)
    y = reference_forward(form, p, xr)
    d = y - target[first].double()
    per = torch.sqrt(d * d + 1e-6).flatten(1).sum(1)                                    # O.charbonnier_loss: mean(sqrt(d^2 + eps^2)), eps 1e-3
    loss = (per * torch.tensor(count, dtype=torch.float64)).sum() / (B * d[0].numel())
    names = [k for k, v in p.items() if v.is_floating_point()]
    grads = torch.autograd.grad(loss, [xr] + [p[k] for k in names], allow_unused=True)
    g = {k: (gr if gr is not None else torch.zeros_like(p[k])) for k, gr in zip(names, grads[1:])}
    dx = torch.stack([grads[0][k] / count[k] for k in where])
    return y.detach()[where], float(loss.detach()), dx, g


def charbonnier_dy(y_ref: Tensor, target: Tensor) -> Tensor:
    """d loss / d y at the reference output (O.charbonnier_loss: eps 1e-3), float32, as tests/test_gpu_win4.py feeds its backward"""
    d = y_ref.double() - target.double()
    return (d / torch.sqrt(d * d + 1e-6) / d.numel()).float()


GRAD_FAULTS = ("grad_zeroed", "grads_swapped", "dx_image_order")


def faulted_grads(fault: str, dx: Tensor, grads: Dict[str, Tensor]):
    """the stand-in faults of the training rows, applied to the reference's gradients; returns (dx, grads, names of the tensors concerned)"""
    g = dict(grads)
    if fault == "grad_zeroed":
        n = "decoderlayer_0.blocks.0.attn.proj.weight"
        g[n] = torch.zeros_like(g[n])
        return dx, g, [n]
    if fault == "grads_swapped":
        a, b = "encoderlayer_1.blocks.0.norm1.weight", "encoderlayer_1.blocks.0.norm2.weight"
        g[a], g[b] = grads[b], grads[a]
        return dx, g, [a, b]
    if fault == "dx_image_order":
        return dx.roll(1, 0), g, ["dx"]                    # (a flip would leave the batch a, b, a as it is)
    raise ValueError(fault)


if __name__ == "__main__":
    for title, rows in (("INFER_ROWS", generate_infer_rows()), ("TRAIN_ROWS", generate_train_rows())):
        print(f"{title}: List[str] = [")
        for r in rows:
            print(f'    "{r}",')
        print("]")
