"""The definition of ALTERED content shared between recordings in plain Python: what shz_shared_warps_peaks /
shz_shared_warps_batch compute.  Nothing of the library is called: the warp is warp_twin.warp_peaks_tf, the pairing
oracle.cpu_ref.pair_keys, the join shared_twin.cells -- on a list of VIRTUAL recordings (the plain ones, then every distinct
(a, v) in the order of its first job), once per distinct window.

All quantities are integers, in frames; lags are signed here (the library returns them biased by 2^20)."""
import numpy as np

import shared_twin
from oracle import cpu_ref as O
from warp_twin import warp_peaks_tf

JOB_KEYS = ("job_pairs", "job_skipped_keys", "job_skipped_rows")
CELL_KEYS = ("lag", "block", "pairs", "first", "last")


def virtual_hashes(peak_f, peak_t, peak_off, rec_clip0, tempos, pitches, jobs, fan_value=5):
    """(key32, t1, hash_off, virt_clip0, virt): the hashes of every clip as it is, then of the clips of every distinct (a, v) of
    the jobs warped by (tempos[v], pitches[v]); virt_clip0 the CSR of the virtual recordings over those clips; virt[(a, v)] the
    virtual recording of the pair."""
    peak_f, peak_t = np.asarray(peak_f, np.int64), np.asarray(peak_t, np.int64)
    n_recs = len(rec_clip0) - 1
    ks, ts, ho = [], [], [0]

    def clip(c, t16=None, f16=None):
        a, b = int(peak_off[c]), int(peak_off[c + 1])
        if t16 is None:                                                         # H_r: the clip as it is
            k, t1 = O.pair_keys(peak_f[a:b], peak_t[a:b], fan_value)
        else:                                                                   # H_{r,v}: warped, at (65536, 65536) too
            k, t1 = O.pair_keys(*warp_peaks_tf(peak_f[a:b], peak_t[a:b], t16, f16), fan_value)
        ks.extend(int(x) for x in k)
        ts.extend(int(x) for x in t1)
        ho.append(len(ks))
    for c in range(int(rec_clip0[n_recs])):
        clip(c)
    virt_clip0 = [int(x) for x in rec_clip0]
    virt = {}
    for job in jobs:
        a, v = int(job[0]), int(job[2])
        if (a, v) in virt:
            continue
        virt[(a, v)] = len(virt_clip0) - 1
        for c in range(int(rec_clip0[a]), int(rec_clip0[a + 1])):
            clip(c, int(tempos[v]), int(pitches[v]))
        virt_clip0.append(len(ho) - 1)
    return ks, ts, ho, virt_clip0, virt


def cells(peak_f, peak_t, peak_off, rec_clip0, tempos, pitches, jobs, max_run, cell_shift, min_cell_pairs, fan_value=5):
    """jobs: a list of (a, b, v, lag_lo, lag_hi).  Returns shared_twin.cells' dict over the jobs (first, last and block in a's
    WARPED frames), rec_hashes over the plain recordings, and job_hashes."""
    n_recs = len(rec_clip0) - 1
    ks, ts, ho, vc0, virt = virtual_hashes(peak_f, peak_t, peak_off, rec_clip0, tempos, pitches, jobs, fan_value)
    vjobs = [(virt[(int(a), int(v))], int(b)) for a, b, v, _, _ in jobs]
    per_window = {}
    for w in {(int(lo), int(hi)) for _, _, _, lo, hi in jobs} or {(0, 0)}:
        per_window[w] = shared_twin.cells(ks, ts, ho, vc0, vjobs, w[0], w[1], max_run, cell_shift, min_cell_pairs)
    any_one = next(iter(per_window.values()))
    out = {k: [] for k in CELL_KEYS + JOB_KEYS}
    out["cell_off"] = [0]
    out["rec_hashes"] = any_one["rec_hashes"][:n_recs]
    out["job_hashes"] = [any_one["rec_hashes"][vj[0]] for vj in vjobs]
    for j, (_, _, _, lo, hi) in enumerate(jobs):
        w = per_window[(int(lo), int(hi))]
        for k in CELL_KEYS:
            out[k].extend(w[k][w["cell_off"][j]:w["cell_off"][j + 1]])
        for k in JOB_KEYS:
            out[k].append(w[k][j])
        out["cell_off"].append(len(out["lag"]))
    return out
