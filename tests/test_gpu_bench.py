"""bench.py end to end on one GPU: the plain run and the torch.distributed.run launch with the
collective path forced on (one rank over RCCL), so the N > 1 plumbing -- process group on the
device, lagged all-gather of the packed rows joined on the collective's stream, max-over-ranks
timing -- is exercised before the driver runs it on 2/4/8 GPUs."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _line(out: str) -> dict:
    rows = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(rows) == 1, out[-2000:]
    return json.loads(rows[0])


def test_bench_single_process_contract():
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--steps", "4", "--warmup", "1", "--batch", "8",
                        "--seconds", "5", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _line(p.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["value"] > 0 and d["roofline"]["bound"] == "mfma"
    assert 0 < d["roofline"]["frac"] < 1
    # HBM traffic is quoted from a committed counter summary only for the shape it was taken at (M = 8064)
    assert d["roofline"]["traffic"] is None and "no committed counter summary" in d["roofline"]["traffic_source"]
    assert d["dtype"] == "f16" and "not a BASELINE.json configuration" in d["config"]["workload"]
    assert d["roofline"]["kernel"].startswith("k_gemm") and "batches in flight" in d["roofline"]["tile_policy"]
    # the verse-shaped replay legs: every transcript passes the text gate / every one fails it
    pl = d["post_logits"]
    assert pl["gate_pass"]["use_ctc_fraction"] == 0.0 and pl["gate_fail"]["use_ctc_fraction"] == 1.0
    assert pl["gate_fail"]["ms_per_batch"] > pl["gate_pass"]["ms_per_batch"] > 0


def test_bench_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """without --full the line carries the headline only (every secondary block null) and --dump-outputs writes the
    rows the timed path returned for its last step, one float64 entry per utterance"""
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                        "--seconds", "5", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _line(p.stdout)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "utterances/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f16"
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    for k in ("roofline", "cpu_baseline", "post_logits", "realistic_mix", "ingest", "long_region", "extra"):
        assert d[k] is None, k
    import numpy as np

    arrs = {f.stem: np.load(f) for f in out.glob("*.npy")}
    assert {"surah", "ayah", "ayah_end", "score", "source", "use_ctc", "t_frames"} <= set(arrs), sorted(arrs)
    assert all(a.dtype == np.float64 and a.shape[0] == 8 for a in arrs.values())
    assert np.isfinite(arrs["score"]).all() and (arrs["t_frames"] == arrs["t_frames"][0]).all() and arrs["t_frames"][0] > 0
    assert d["config"]["gate_failed_utterances_per_batch"] == int(arrs["use_ctc"].sum())


def _own_queues_env() -> dict:
    """the caller's environment without GPU_MAX_HW_QUEUES, so that the child runs on the hardware queues the package
    exports (8) and not on whatever the calling shell chose: the four-context assertions below are about that setup"""
    return {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}


def test_bench_tta30_workload_small():
    """--workload tta30 (BASELINE configs[4]) at a reduced size: anchor pass, gate, GPU-resampled copies,
    decision rule; seeded random weights gate every clip."""
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--workload", "tta30", "--steps", "2", "--warmup", "1",
                        "--batch", "4", "--seconds", "6", "--no-cpu-baseline", "--no-post-logits"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=_own_queues_env())
    assert p.returncode == 0, p.stderr[-2000:]
    d = _line(p.stdout)
    assert "TTA" in d["metric"] and d["config"]["tta_gated_fraction"] == 1.0 and d["value"] > 0
    assert "configs[4]" in d["config"]["workload"] and d["config"]["batches_in_flight"] == 4


def test_bench_tta30_with_the_reference_gate_ratio_small():
    """--tta-mix: the anchor pass reads verse-shaped log-probs at the v1 run's 46 : 7 branch ratio, so only about one clip in
    eight fails the 0.5 gate and gets its 0.9x / 1.1x copies (seeded random weights alone gate every clip)."""
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--workload", "tta30", "--tta-mix", "--steps", "3", "--warmup", "1",
                        "--batch", "16", "--seconds", "8", "--no-cpu-baseline", "--no-post-logits"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _line(p.stdout)
    assert "TTA" in d["metric"] and d["value"] > 0
    assert 0.0 < d["config"]["tta_gated_fraction"] <= 0.25, d["config"]["tta_gated_fraction"]


def test_bench_under_torchrun_with_collective_path():
    env = dict(os.environ, QVERSE_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29731", str(ROOT / "bench.py"), "--full", "--gpus", "1",
                        "--steps", "5", "--warmup", "2", "--batch", "8", "--seconds", "5", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    d = _line(p.stdout)
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["config"]["batches_in_flight"] == 4


def test_bench_tta30_under_torchrun_with_collective_path():
    """configs[4]'s workload through the torch.distributed path (one rank, collective forced on): anchor pass, gate, the
    GPU-resampled copies, the decision rule, then the combined rows packed on the host and all-gathered over RCCL on the
    side stream (bench.py tta_done) -- the one multi-GPU path no test had executed."""
    env = dict(os.environ, QVERSE_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29733", str(ROOT / "bench.py"), "--full", "--gpus", "1",
                        "--workload", "tta30", "--steps", "3", "--warmup", "1", "--batch", "4", "--seconds", "6",
                        "--no-cpu-baseline", "--no-post-logits"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    d = _line(p.stdout)
    assert d["n_gpus"] == 1 and d["value"] > 0 and "TTA" in d["metric"]
    assert d["config"]["tta_gated_fraction"] == 1.0 and d["config"]["batches_in_flight"] == 4


_CTX_PROG = r"""
import os, sys, json, time
sys.path.insert(0, %r); sys.path.insert(0, %r)
os.environ.pop("GPU_MAX_HW_QUEUES", None)
late = sys.argv[1] == "late"
import torch
if late:   # a host application that touched HIP before the package could export GPU_MAX_HW_QUEUES
    torch.zeros(8, device="cuda").sum().item()
import offline_tarteel_amd
from offline_tarteel_amd.engine import Engine
from synth import synth_audio
eng = Engine(device=0, with_model=True, seed=20260630, max_batch=64, max_samples=160000, contexts=4)
a = torch.from_numpy(synth_audio(64, 160000, seed=5)).cuda().contiguous()
lens = [160000] * 64
best = 0.0
for rep in range(3):
    for _ in range(6): eng.predict_batch_async(a, lens)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(40): eng.predict_batch_async(a, lens)
    torch.cuda.synchronize()
    best = max(best, 64 * 40 / (time.perf_counter() - t0))
print(json.dumps({"contexts": eng.contexts, "probe": int(eng.lib.qv_probe_concurrent_streams()), "utt_per_s": best}))
eng.close()
"""


def test_batches_in_flight_do_not_depend_on_who_initialised_hip_first():
    """GPU_MAX_HW_QUEUES is read once, when HIP initialises.  A host that touched torch.cuda before importing the package
    runs on the runtime's default (4 hardware queues), where four context streams share queues and lose ~14 %; qv_create
    measures how many streams really run side by side (qv_probe_concurrent_streams) and falls back to three batches in
    flight, the best setting there.  The late-initialised process must stay within a few per cent of the normal one."""
    prog = _CTX_PROG % (str(ROOT), str(ROOT / "tests"))
    res = {}
    for mode in ("early", "late"):
        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        p = subprocess.run([sys.executable, "-c", prog, mode], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        res[mode] = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    print("[contexts]", res)
    assert res["early"]["contexts"] == 4 and res["early"]["probe"] == 4, res
    assert res["late"]["contexts"] == 3 and res["late"]["probe"] < 4, res
    assert res["late"]["utt_per_s"] >= 0.92 * res["early"]["utt_per_s"], res


def test_engine_created_before_any_other_device_work_runs_at_full_speed():
    """A process whose FIRST device work is qv_create (a host binding libqverse.so directly; tools/sweep.py) used to run a
    four-context engine at 4.7-4.8 ms per batch instead of 3.5: the default stream, which every batch is ordered behind,
    got its hardware queue after the engine's streams and shared one with a context.  qv_create now runs a kernel on it
    first.  Two fresh processes, engine first / torch first: the same rate (the old gap was 37 %; 12 % is allowed)."""
    import subprocess

    def run(order):
        out = subprocess.run([sys.executable, str(ROOT / "tools" / "init_order_probe.py"), order, "--steps", "40"],
                             capture_output=True, text=True, timeout=300, cwd=str(ROOT), env=_own_queues_env())
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    a, b = run("engine_first"), run("torch_first")
    assert a["contexts"] == b["contexts"] == 4
    assert a["ms_per_batch"] < 1.12 * b["ms_per_batch"], (a, b)


def test_bench_strong2048_under_torchrun_with_the_sharded_gather():
    """--workload strong2048 with the collective path forced on for one rank: dist.shard_plan deals the ragged global batch
    of 2,048 clips (5-30 s), the rank's share runs in engine calls of 64 with batches in flight, dist.all_gather_results
    un-permutes the rows over RCCL -- the functions the sharded runner entry ships, at the size of BASELINE configs[3]."""
    env = dict(os.environ, QVERSE_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29563", str(ROOT / "bench.py"), "--full", "--gpus", "1",
                        "--workload", "strong2048", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-post-logits"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _line(p.stdout)
    assert d["scaling"] == "strong" and d["config"]["global_batch"] == 2048 and d["value"] > 0
    assert d["config"]["deal"] == "strided" and d["audio_seconds_per_s"] > 0
    assert "shard_plan" in d["config"]["workload"]


def test_bench_ingest_leg_small():
    """the `ingest` leg of the default line at a reduced size: distinct pinned host batches cross PCIe on a copy stream into a ring
    of device buffers one step ahead of the engine; every timed forward is accounted for (graph replays + plain launches)."""
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--steps", "10", "--warmup", "2", "--batch", "8",
                        "--seconds", "5", "--no-cpu-baseline", "--no-extra"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _line(p.stdout)
    ing = d["ingest"]
    assert "error" not in ing, ing
    assert ing["value"] > 0 and ing["host_batches"] == 8 and ing["device_buffers"] == d["config"]["batches_in_flight"] + 2
    assert ing["forward_graph"]["forwards"] == 30 and ing["forward_graph"]["replays"] >= 20
    assert ing["h2d_gb_per_s"] > 0
