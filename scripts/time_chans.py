#!/usr/bin/env python3
"""Time the stem and head kernels at image channel counts other than 3, and whole Uformer-B models 6 -> 3 and 4 -> 4 beside 3 -> 3.

  * stem (uf_input_proj_fwd): the LDS-staged second form against the first form (UF_VARIANT="stem=1", the route these shapes took before the second
    form was built for them) at Cin in {1, 3, 4, 6}, E = 32, 16 x 256 x 256;
  * head (uf_output_proj_c_fwd): Cout in {1, 4} against Cout = 3 at C2 = 64, 16 x 256 x 256;
  * model: Uformer-B 6 -> 3 and 4 -> 4 at 256 x 256, batch 16, bf16, next to 3 -> 3 in the same process.

HIP-event timing; the variants alternate inside one process and every figure is kept per repeat, so the run-to-run spread is in the file next to the
ratio it qualifies.

    python scripts/time_chans.py [--out profiles/chans_fwd.json] [--steps 50] [--repeats 5]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from uformer_amd import model, ops, spec  # noqa: E402


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def alternate(fns, steps, repeats):
    """{name: [ms per repeat]} with the variants taking turns inside every repeat"""
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(timed(fn, steps))
    return out


def stats(ms):
    med = statistics.median(ms)
    return {"ms": ms, "ms_median": med, "spread": (max(ms) - min(ms)) / med}


def with_variant(value, fn):
    def run():
        old = os.environ.get("UF_VARIANT")
        if value is None:
            os.environ.pop("UF_VARIANT", None)
        else:
            os.environ["UF_VARIANT"] = value
        try:
            return fn()
        finally:
            if old is None:
                os.environ.pop("UF_VARIANT", None)
            else:
                os.environ["UF_VARIANT"] = old
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chans_fwd.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    res = {"batch": B, "H": S, "W": S, "gpu": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats, "stem_rows": [], "head_rows": [],
           "model_rows": []}
    gen = torch.Generator().manual_seed(1)
    E = 32
    for Cin in (1, 3, 4, 6):
        img = torch.rand(B, Cin, S, S, generator=gen).cuda()
        w27, bias = torch.randn(Cin * 9, E, generator=gen).cuda(), torch.randn(E, generator=gen).cuda()
        fns = {"first": with_variant("stem=1", lambda: ops.input_proj(img, w27, bias)), "second": with_variant("stem=2", lambda: ops.input_proj(img, w27, bias))}
        assert torch.equal(fns["first"](), fns["second"]()), "the two forms differ"
        t = alternate(fns, args.steps, args.repeats)
        row = {"Cin": Cin, "E": E, "first": stats(t["first"]), "second": stats(t["second"])}
        row["second_over_first"] = row["second"]["ms_median"] / row["first"]["ms_median"]
        row["second_out_gbs"] = 4.0 * B * S * S * E / row["second"]["ms_median"] / 1e6
        print(json.dumps(row), flush=True)
        res["stem_rows"].append(row)
    C2 = 64
    rows = torch.randn(B * S * S, C2, generator=gen).cuda()
    heads = {}
    for Cout in (1, 3, 4):
        w, bias = torch.randn(Cout, 9, C2, generator=gen).cuda(), torch.randn(Cout, generator=gen).cuda()
        heads[Cout] = (lambda w=w, bias=bias: ops.output_proj(rows, w, bias, B, S, S))
    t = alternate(heads, args.steps, args.repeats)
    for Cout in (1, 3, 4):
        row = {"Cout": Cout, "C2": C2, **stats(t[Cout])}
        row["over_cout3"] = row["ms_median"] / statistics.median(t[3])
        row["in_gbs"] = 4.0 * B * S * S * C2 / row["ms_median"] / 1e6
        print(json.dumps(row), flush=True)
        res["head_rows"].append(row)
    del rows
    if not args.no_model:
        models, xs = {}, {}
        with torch.no_grad():
            for dd_in, in_chans in ((3, 3), (6, 3), (4, 4)):
                cfg = dataclasses.replace(spec.arch_config("Uformer_B", img_size=S), dd_in=dd_in, in_chans=in_chans)
                m = model.Uformer(img_size=S, in_chans=in_chans, dd_in=dd_in, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                                  modulator=True, compute_dtype=torch.bfloat16).eval()
                m.load_state_dict(spec.synth_state_dict(cfg, 1234), strict=True)
                key = f"{dd_in}->{in_chans}"
                models[key], xs[key] = m.cuda(), spec.synth_input(B, S, S, 1234, channels=dd_in).cuda()
            t = alternate({k: (lambda k=k: models[k](xs[k])) for k in models}, max(5, args.steps // 5), args.repeats)
        for k in models:
            row = {"model": "Uformer_B " + k, "dtype": "bfloat16", **stats(t[k])}
            row["img_s"] = B * 1000.0 / row["ms_median"]
            print(json.dumps(row), flush=True)
            res["model_rows"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
