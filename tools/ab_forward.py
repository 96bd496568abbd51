#!/usr/bin/env python
"""dev: dump the log-probs of a ragged seeded batch (compare two builds / env switches bitwise).

    python tools/ab_forward.py OUT.pt [--variant N] [--precision P] [--gemm-tiles T] [--gemm-tile-height H] [--frames T [T ...]]

One utterance per frame count.  The default counts are the tile edges of the attention kernels (32-key tiles, 128-query
groups; tests/test_gpu_forward.py) and 376: 12 key tiles and three query groups, so both position rings (192 and 256 rows)
and both stage counts of the key-tiled kernels wrap more than once.  --variant is Engine.attention_variant, --precision
the engine's precision mode (0 f16, 1 int4 / int8 weights, 2 int8 activations too), --gemm-tiles / --gemm-tile-height
Engine.gemm_tiles / gemm_tile_height (0 = 128-wide only, 1 = default, 2 = 256 x 256 wherever the shape allows; height
3 = 192 rows always): between them every GEMM instantiation can be put under a forward."""
import argparse
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch
import offline_tarteel_amd  # noqa
from offline_tarteel_amd.engine import Engine
from forward_ref import samples_for_frames
from synth import synth_audio
ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--variant", type=int, default=None)
ap.add_argument("--precision", type=int, choices=(0, 1, 2), default=0)
ap.add_argument("--gemm-tiles", type=int, choices=(0, 1, 2), default=None)
ap.add_argument("--gemm-tile-height", type=int, default=None)
ap.add_argument("--frames", type=int, nargs="+", default=[1, 31, 32, 33, 64, 65, 127, 128, 129, 160, 255, 256, 257, 376])
args = ap.parse_args()
lens = [samples_for_frames(t) for t in args.frames]
a = torch.from_numpy(synth_audio(len(lens), max(lens), seed=5))
for b, n in enumerate(lens):
    a[b, n:] = 0
eng = Engine(device=0, with_model=True, seed=3, precision=args.precision, max_batch=len(lens), max_samples=max(lens))
if args.gemm_tiles is not None:
    eng.gemm_tiles(args.gemm_tiles)
if args.gemm_tile_height is not None:
    eng.gemm_tile_height(args.gemm_tile_height)
if args.variant is not None:
    eng.attention_variant(args.variant)
lp, t = eng.forward(a.cuda().contiguous(), lens)
assert t == args.frames, (t, args.frames)
torch.save({"lp": lp.cpu(), "t": t}, args.out)
print("saved", args.out, t)
