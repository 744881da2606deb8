"""bench.py's command line: a plain run times ONE region of exactly --steps steps and carries only the headline; --full brings back the
repeated regions and every companion measurement; --dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_plain_run_times_exactly_steps_in_one_region():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.steps, a.warmup, a.repeats, a.dump_outputs) == (False, 7, 2, 1, None)


def test_full_keeps_the_repeated_regions():
    a = bench.parse_args(["--full"])
    assert a.full and a.repeats == 7
    assert bench.parse_args(["--full", "--repeats", "3"]).repeats == 3


@pytest.mark.parametrize("flag", [["--kernels-json", "k.json"], ["--error-budget"]])
def test_full_only_options_are_refused_without_full(flag):
    with pytest.raises(SystemExit):
        bench.parse_args(flag)
    assert bench.parse_args(["--full"] + flag).full


def test_dump_outputs_writes_float32(tmp_path):
    y = torch.rand(3, 3, 8, 8, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    info = bench.dump_outputs(y, str(tmp_path / "d"))
    z = np.load(tmp_path / "d" / "restored.npy")
    assert z.dtype == np.float32 and z.shape == (3, 3, 8, 8) and info["restored"]["shape"] == [3, 3, 8, 8]
    assert np.array_equal(z, y.float().numpy())


def test_dump_outputs_keeps_the_leading_images_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 2 * 3 * 8 * 8 * 4)
    y = torch.rand(5, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    bench.dump_outputs(y, str(tmp_path))
    z = np.load(tmp_path / "restored.npy")
    assert z.shape == (2, 3, 8, 8) and np.array_equal(z, y[:2].numpy())


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_timed_forward(tmp_path):
    """A plain run on a small model: one JSON line with the headline fields, exactly --steps timed steps, and restored.npy equal bit for bit
    to the same forward run here (seeded weights and inputs; the forward is deterministic: tests/test_gpu_model.py)."""
    from uformer_amd import spec
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--arch", "tiny32", "--img", "128",
           "--batch", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["repeats"] == 1 and not d["full"] and len(d["region_ms_per_step"]) == 1
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert not {"roofline", "cpu_baseline", "parity", "vendor_baseline", "kernels"} & set(d)
    got = np.load(tmp_path / "restored.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 128, 128)
    cfg = spec.arch_config("tiny32", img_size=128)
    m = bench.build_model(None, cfg, spec.synth_state_dict(cfg, 1234), torch.device("cuda", 0), torch.bfloat16)
    with torch.no_grad():
        want = m(spec.synth_input(2, 128, 128, 1234).cuda()).float().cpu().numpy()
    assert np.array_equal(got, want)
