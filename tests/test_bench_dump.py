"""bench.py --dump-outputs (the last timed step's outputs as .npy files), the meaning of --steps / ms_per_step, and what a plain run (no --full)
leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from hyslam_amd import _native as N  # noqa: E402


def _buffers(B, cap, n_l, n_r, seed=0):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(seed)
    kp = np.zeros((2, B, cap), N.KP_DTYPE)
    for f in ("x", "y", "size", "angle", "response"):
        kp[f] = rng.uniform(0, 1000, (2, B, cap)).astype(np.float32)
    kp["octave"] = rng.integers(0, 8, (2, B, cap))
    desc = rng.integers(0, 256, (2, B, cap, 32), dtype=np.uint8)
    uR, depth = rng.uniform(-1, 1900, (2, B, cap)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())
    bufs = dict(kL=t(kp[0]), dL=t(desc[0]), nL=torch.tensor(n_l, dtype=torch.int32), kR=t(kp[1]), dR=t(desc[1]),
                nR=torch.tensor(n_r, dtype=torch.int32), uR=torch.from_numpy(uR.reshape(-1).copy()), depth=torch.from_numpy(depth.reshape(-1).copy()))
    return bufs, kp, desc, uR, depth


def test_dump_holds_the_valid_prefix_of_every_pair(tmp_path):
    B, cap = 3, 50
    n_l, n_r = [50, 0, 17], [3, 49, 20]
    b, kp, desc, uR, depth = _buffers(B, cap, n_l, n_r)
    P = bench.dump_outputs(str(tmp_path), N, cap, b["kL"], b["dL"], b["nL"], b["kR"], b["dR"], b["nR"], b["uR"], b["depth"])
    assert P == B
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"n_left", "n_right", "keypoints_left", "keypoints_right", "descriptors_left", "descriptors_right", "u_right", "depth"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["n_left"].tolist() == n_l and got["n_right"].tolist() == n_r
    for side, n, k, d in (("left", n_l, kp[0], desc[0]), ("right", n_r, kp[1], desc[1])):
        rows = np.concatenate([k[j, :n[j]] for j in range(B)])
        want = np.stack([rows[f].astype(np.float64) for f in N.KP_DTYPE.names], axis=1)
        assert np.array_equal(got["keypoints_" + side], want)
        assert np.array_equal(got["descriptors_" + side], np.concatenate([d[j, :n[j]] for j in range(B)]).astype(np.float32))
    assert np.array_equal(got["u_right"], np.concatenate([uR[j, :n_l[j]] for j in range(B)]))
    assert np.array_equal(got["depth"], np.concatenate([depth[j, :n_l[j]] for j in range(B)]))


def test_dump_stays_within_64_mb_by_a_fixed_pair_count(tmp_path):
    B, cap = 64, 4096
    b = _buffers(B, cap, [cap] * B, [cap] * B)[0]
    P = bench.dump_outputs(str(tmp_path), N, cap, b["kL"], b["dL"], b["nL"], b["kR"], b["dR"], b["nR"], b["uR"], b["depth"])
    assert 0 < P < B
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    assert np.load(tmp_path / "n_left.npy").shape == (P,)


def test_dump_refuses_counts_outside_the_buffers(tmp_path):
    b = _buffers(2, 10, [10, 11], [0, 0])[0]
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path), N, 10, b["kL"], b["dL"], b["nL"], b["kR"], b["dR"], b["nR"], b["uR"], b["depth"])


def test_steps_are_single_passes_by_default_and_dump_is_c2_only(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    a = bench.parse_args()
    assert a.steps == 7 and a.min_timed_ms == 0 and a.dump_outputs == ""
    assert a.full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full is True
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "c3", "--dump-outputs", "x"])
    with pytest.raises(SystemExit):
        bench.parse_args()


@pytest.mark.gpu
def test_bench_dumps_the_last_step(gpu, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--pairs", "4", "--full", "--cpu-seconds", "0",
                        "--pcie-seconds", "0", "--call-site", "0", "--latency-calls", "0", "--copy-gib", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["inner_repeats"] == 1 and line["ms_per_step"] > 0
    assert abs(line["ms_per_step"] * 4 - line["timed_region_ms"]) <= 0.01 * line["timed_region_ms"] + 0.2
    assert line["parity_checksum_ok"] is True and line["outputs_dumped"]["pairs"] == 4
    n_l, n_r = np.load(out / "n_left.npy"), np.load(out / "n_right.npy")
    assert n_l.shape == (4,) and (n_l > 0).all()
    assert np.load(out / "keypoints_left.npy").shape == (int(n_l.sum()), 6) and np.load(out / "descriptors_right.npy").shape == (int(n_r.sum()), 32)
    assert np.load(out / "depth.npy").shape == (int(n_l.sum()),) and (np.load(out / "depth.npy") > 0).sum() > 100
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20


# what --full adds to the C2 line; a plain run carries none of it
FULL_ONLY = ("parity_checksum_ok", "pairs_checked", "parity_checksum", "measured_copy_peak", "latency_one_pair_ms", "latency_one_pair", "pcie_inclusive",
             "call_site", "cpu_baseline", "rccl")


@pytest.mark.gpu
def test_plain_run_does_only_the_headline(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "2"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["value"] > 0 and line["steps"] == 3 and line["warmup"] == 1 and line["roofline"]["frac"] > 0
    assert not [k for k in FULL_ONLY if k in line]
    assert "peak_measured_copy" not in line["roofline"] and "peak_measured_copy" not in line["end_to_end"]
