"""Resampling of 1,000 x 30 s clips at 48 kHz to 44.1 kHz, device resident, beside the extraction of its own output in the
same process: the kernel timers of the context (shz_get_kernel_ms) for both, median of the repeats after a warm-up.
python scripts/resample_bench.py [--clips 1000] [--seconds 30] [--fs-in 48000] [--repeats 7]"""
import argparse
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from shazam_amd import _ffi  # noqa: E402
from shazam_amd.resample import out_len, resample_plan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=1000)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--fs-in", type=int, default=48000)
ap.add_argument("--fs-out", type=int, default=44100)
ap.add_argument("--repeats", type=int, default=7)
a = ap.parse_args()

ctx = _ffi.Context(0)
nc, n = a.clips, int(a.seconds * a.fs_in)
L, M, T, taps = resample_plan(a.fs_in, a.fs_out)
n_out = out_len(n, L, M)
pcm = ctx.synth_corpus(1, 4321, 0, nc, n)          # music-like tracks, generated at the input rate's sample count
off = np.arange(nc + 1, dtype=np.uint64) * n
out = ctx.alloc(nc * n_out * 2)
off_out = np.arange(nc + 1, dtype=np.uint64) * n_out
cap = nc * (n_out // 2048 + 1) * 40
kb, tb = ctx.alloc(cap * 4), ctx.alloc(cap * 4)


def resample():
    rc, _, oo, cnt = ctx.resample_raw(pcm, off, L, M, T, taps, pcm_device=True, out=out)
    ctx.check(rc)
    assert cnt == nc * n_out and np.array_equal(oo, off_out)


def extract():
    return ctx.fingerprint_batch(out, off_out, fs=a.fs_out, pcm_device=True, out_key=kb, out_t1=tb, cap=cap)[3]


resample()       # warm-up of both, unprofiled
extract()
rs_ms, ex_ms, ex_kernels = [], [], []
for _ in range(a.repeats):
    ctx.set_profiling(True)
    resample()
    rs_ms.append(ctx.resample_kernel_ms()[0])
    ctx.set_profiling(True)      # (zeroes the timers)
    hashes = extract()
    k = {nm: v[0] for nm, v in ctx.kernel_ms().items()}
    ex_kernels.append(k)
    ex_ms.append(sum(k.values()))
ctx.set_profiling(False)
rs, ex = statistics.median(rs_ms), statistics.median(ex_ms)
gb = (nc * n * 2 + nc * n_out * 2) / 1e9
print(json.dumps({
    "clips": nc, "seconds": a.seconds, "fs_in": a.fs_in, "fs_out": a.fs_out, "L": L, "M": M, "T": T,
    "resample_kernel_ms": round(rs, 3), "resample_kernel_ms_all": [round(v, 3) for v in rs_ms],
    "resample_gb_moved": round(gb, 3), "resample_gb_per_s": round(gb / (rs * 1e-3), 1),
    "extract_kernels_ms": round(ex, 3), "extract_kernels_ms_all": [round(v, 3) for v in ex_ms],
    "extract_kernels_split_ms": {nm: round(statistics.median(k[nm] for k in ex_kernels), 3) for nm in ex_kernels[0]},
    "hashes": int(hashes), "resample_below_extract": bool(rs < ex), "device": ctx.device_info()["name"]}))
for b in (pcm, out, kb, tb):
    b.free()
