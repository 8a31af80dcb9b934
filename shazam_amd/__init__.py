"""shazam_amd -- the fingerprint / recognise hot path of CarlosArturoMe/shazam on MI355X.

Host side is Python + numpy + ctypes over the C ABI of ``libshz.so`` (``include/shz.h``);
every stage runs as hand-written HIP on the GPU.  There is NO CPU fallback: importing works
anywhere, but the first call needs the built library and a ROCm GPU and raises otherwise.

The functions below keep the reference's names, arguments and return types
(``__init__.py:116-245`` = ``recognizer.py:86-212`` for extraction, ``recognizer.py:222-338``
for match/align, ``__init__.py:24-27,54-67`` for the database registry) so this package can
be dropped in behind them; ``fingerprint_batch`` / ``recognize_batch`` are the batched forms
the GPU wants.
"""
from __future__ import annotations

import importlib
from operator import itemgetter
from time import time

import numpy as np

from . import _ffi
from ._ffi import HOP, NFFT, Context, ShzError, Table, takes_delta_tol, takes_key_cap, takes_song_filter  # noqa: F401

# reference constants (__init__.py:41-51, recognizer.py:21-38,40-58,68)
RATE = 44100
DEFAULT_FS = 44100
DEFAULT_WINDOW_SIZE = 4096
DEFAULT_OVERLAP_RATIO = 0.5
DEFAULT_FAN_VALUE = 5
DEFAULT_AMP_MIN = 10
CONNECTIVITY_MASK = 2
PEAK_NEIGHBORHOOD_SIZE = 10
PEAK_SORT = True
MIN_HASH_TIME_DELTA = 0
MAX_HASH_TIME_DELTA = 200
FINGERPRINT_REDUCTION = 20
TOPN = 2
FIELD_FILE_SHA1 = "file_sha1"
SONG_ID = "song_id"
SONG_NAME = "song_name"
FIELD_TOTAL_HASHES = "total_hashes"
INPUT_HASHES = "input_total_hashes"
INPUT_CONFIDENCE = "input_confidence"
FINGERPRINTED_HASHES = "fingerprinted_hashes_in_db"
HASHES_MATCHED = "hashes_matched_in_input"
FINGERPRINTED_CONFIDENCE = "fingerprinted_confidence"
OFFSET = "offset"
OFFSET_SECS = "offset_seconds"

# the reference's own plugin registry (__init__.py:24-27) with the HIP table added
DATABASES = {
    "hip": ("shazam_amd.db", "HipFingerprintDB"),
    "mysql": ("mysql_database", "MySQLDatabase"),
    "postgres": ("dejavu.database_handler.postgres_database", "PostgreSQLDatabase"),
}


def get_database(database_type: str = "hip"):
    """__init__.py:54-67: class for a registry key; unknown/unimportable -> TypeError."""
    try:
        path, db_class_name = DATABASES[database_type]
        return getattr(importlib.import_module(path), db_class_name)
    except (ImportError, KeyError):
        raise TypeError("Unsupported database type supplied.")


_ctx = None


def get_context(device_id: int | None = None) -> Context:
    """Process-wide default context (device from SHZ_DEVICE / LOCAL_RANK, else 0)."""
    global _ctx
    if _ctx is None:
        import os
        if device_id is None:
            device_id = int(os.environ.get("SHZ_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _ctx = Context(device_id)
    return _ctx


# hex20 -> key32 of every hash this process has produced, so the hex-keyed reference API
# (insert_hashes / return_matches) can address the key-indexed device table.
_HEX2KEY: dict = {}


def hex_of_keys(ctx: Context, key32: np.ndarray) -> list:
    """sha1(f"{f1}|{f2}|{dt}")[:20] (lower-case hex) of packed keys, computed on the GPU."""
    key32 = np.ascontiguousarray(key32, np.uint32)
    uniq, inv = np.unique(key32, return_inverse=True)
    h = ctx.sha1_prefix(uniq).tobytes().hex()
    hexes = [h[i:i + 20] for i in range(0, len(h), 20)]
    _HEX2KEY.update(zip(hexes, uniq.tolist()))
    return [hexes[i] for i in inv.tolist()]


def keys_of_hexes(hexes, ctx: Context = None, strict: bool = True) -> np.ndarray:
    """key32 of hex hashes.  Hashes this process produced come from the cache; any other (a MySQL
    dump, another process) is inverted on the GPU by hashing the whole 8.4e8-string preimage space
    (shz_sha1_invert).  Raises KeyError for strings that are not a hash of any (f1, f2, dt)."""
    hexes = [h.lower() for h in hexes]
    out = np.empty(len(hexes), np.uint32)
    missing = []
    for i, h in enumerate(hexes):
        k = _HEX2KEY.get(h)
        if k is None:
            missing.append(i)
        else:
            out[i] = k
    if missing:
        uniq = sorted({hexes[i] for i in missing})
        try:
            dig = np.frombuffer(bytes.fromhex("".join(uniq)), np.uint8).reshape(-1, 10)
        except ValueError:
            raise KeyError("hashes must be 20 hex characters (FINGERPRINT_REDUCTION, __init__.py:51)")
        keys = (ctx or get_context()).sha1_invert(dig)
        bad = [u for u, k in zip(uniq, keys.tolist()) if k == 0xFFFFFFFF]
        if bad and strict:
            raise KeyError(f"{len(bad)} hash(es) are not sha1(f1|f2|dt)[:20] of any peak pair, e.g. {bad[0]!r}")
        found = dict(zip(uniq, keys.tolist()))
        _HEX2KEY.update((u, k) for u, k in found.items() if k != 0xFFFFFFFF)
        for i in missing:
            out[i] = found[hexes[i]]   # 0xFFFFFFFF (matches no table row) for non-hashes when not strict
    return out


def key_of_hex(hexstr: str) -> int:
    return int(keys_of_hexes([hexstr])[0])


def _as_pcm(channel_samples) -> np.ndarray:
    x = np.asarray(channel_samples)
    if x.ndim != 1:
        raise ValueError("channel_samples must be 1-D")
    if x.dtype == np.int16:
        return np.ascontiguousarray(x)
    if x.dtype.kind in "iu" or x.size == 0:
        if x.size and (x.min() < -32768 or x.max() > 32767):
            raise NotImplementedError("the HIP path takes 16-bit PCM; samples outside int16 range")
        return np.ascontiguousarray(x.astype(np.int16))
    raise NotImplementedError(f"the HIP path takes 16-bit integer PCM, got dtype {x.dtype}")


def _check_window(wsize, wratio) -> int:
    """noverlap = int(wsize * wratio) as fingerprint() hands it to mlab.specgram (__init__.py:232-237)."""
    noverlap = int(int(wsize) * float(wratio))
    if noverlap >= int(wsize):   # what mlab.specgram raises for this call (mlab:242)
        raise ValueError("noverlap must be less than NFFT")
    if noverlap < 0:
        raise ValueError("wratio must not be negative")
    w = int(wsize)
    if w != DEFAULT_WINDOW_SIZE and (w < 64 or w > 2048 or (w & (w - 1))):
        raise NotImplementedError("window sizes: 4096 (the reference's own, the fast kernel) and the powers of two 64 .. 2048 (a "
                                  "generic GPU spectrogram); 8192 has no packed key (key32 gives a frequency 12 bits), other sizes "
                                  "are not implemented, and there is no CPU fallback")
    return noverlap


def fingerprint_batch(clips, Fs: int = RATE, fan_value: int = DEFAULT_FAN_VALUE, amp_min=DEFAULT_AMP_MIN, ctx: Context = None,
                      wratio: float = DEFAULT_OVERLAP_RATIO, resample_to: int = None):
    """Batched fingerprint(): clips = list of 1-D int16 arrays (or a 2-D array).
    Returns (key32, t1, hash_off): hashes of clip c are [hash_off[c], hash_off[c+1]).
    resample_to: the clips are at Fs and the table at resample_to -- they are resampled on the device (shz_resample_i16) and
    fingerprinted there at Fs = resample_to; the resampled PCM never visits the host."""
    ctx = ctx or get_context()
    if resample_to is not None and int(resample_to) != int(Fs):
        buf, off = resample_to_device(clips, int(Fs), int(resample_to), ctx)
        try:
            return _fingerprint_device(buf, off, int(resample_to), fan_value, amp_min, ctx, wratio)
        finally:
            buf.free()
    noverlap = _check_window(DEFAULT_WINDOW_SIZE, wratio)
    if NFFT - noverlap != getattr(ctx, "hop", HOP):
        ctx.set_overlap(noverlap)
        try:
            return fingerprint_batch(clips, Fs, fan_value, amp_min, ctx, wratio)
        finally:
            ctx.set_overlap(NFFT - HOP)
    arrs = [_as_pcm(c) for c in clips]
    off = np.zeros(len(arrs) + 1, np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    pcm = np.concatenate(arrs) if arrs else np.zeros(0, np.int16)
    if pcm.size == 0:
        pcm = np.zeros(1, np.int16)
    k, t1, ho, _ = ctx.fingerprint_batch(pcm, off, fs=int(Fs), amp_min=float(amp_min), fan_value=int(fan_value))
    return k, t1, ho


def _fingerprint_device(buf, off, Fs, fan_value, amp_min, ctx, wratio):
    """fingerprint_batch of device-resident clips (buf: DevBuf of int16, off: sample offsets)."""
    noverlap = _check_window(DEFAULT_WINDOW_SIZE, wratio)
    other_hop = NFFT - noverlap != getattr(ctx, "hop", HOP)
    if other_hop:
        ctx.set_overlap(noverlap)
    try:
        k, t1, ho, _ = ctx.fingerprint_batch(buf, off, fs=int(Fs), amp_min=float(amp_min), fan_value=int(fan_value), pcm_device=True)
        return k, t1, ho
    finally:
        if other_hop:
            ctx.set_overlap(NFFT - HOP)


def fingerprint(channel_samples, Fs: int = RATE, wsize: int = DEFAULT_WINDOW_SIZE, wratio: float = DEFAULT_OVERLAP_RATIO,
                fan_value: int = DEFAULT_FAN_VALUE, amp_min: int = DEFAULT_AMP_MIN, resample_to: int = None):
    """__init__.py:212-245: FFT the channel, log transform, local maxima, pair hashes.
    Returns list[(hex20, t1)] in the reference's generation order.  resample_to: see fingerprint_batch; it goes with the
    window size 4096 only (NotImplementedError otherwise: resample_batch first, then fingerprint(wsize=...))."""
    noverlap = _check_window(wsize, wratio)
    ctx = get_context()
    if resample_to is not None and int(resample_to) != int(Fs):
        if int(wsize) != DEFAULT_WINDOW_SIZE:
            raise NotImplementedError("resample_to goes with the window size 4096")
        k, t1, _ = fingerprint_batch([channel_samples], Fs, fan_value, amp_min, ctx, wratio, resample_to)
        return list(zip(hex_of_keys(ctx, k), t1.tolist()))
    if int(wsize) != DEFAULT_WINDOW_SIZE:
        # another window size: the reference's own composition (__init__.py:232-245) of GPU stages -- generic spectrogram,
        # get_2D_peaks on the dB array, generate_hashes on the peaks
        arr2D = ctx.stft_db_any(_as_pcm(channel_samples), int(Fs), int(wsize), noverlap)
        return generate_hashes(get_2D_peaks(arr2D, plot=False, amp_min=amp_min), fan_value=fan_value)
    k, t1, _ = fingerprint_batch([channel_samples], Fs, fan_value, amp_min, ctx, wratio)
    return list(zip(hex_of_keys(ctx, k), t1.tolist()))


def get_2D_peaks(arr2D, plot: bool = False, amp_min: int = DEFAULT_AMP_MIN):
    """__init__.py:116-177: list[(freq, time)] of the 21x21 local maxima above amp_min,
    in np.where order (freq asc, time asc)."""
    if plot:
        raise NotImplementedError("plotting is out of scope of the HIP path")
    f, t = get_context().peaks_from_db(np.asarray(arr2D, np.float64), float(amp_min))
    return list(zip(f.astype(np.int64), t.astype(np.int64)))


def generate_hashes(peaks, fan_value: int = DEFAULT_FAN_VALUE):
    """__init__.py:179-210: sorts ``peaks`` in place by time (stable) like the reference, then
    pairs every peak with its next fan_value-1 successors (0 <= dt <= 200)."""
    if PEAK_SORT:
        peaks.sort(key=itemgetter(1))
    ctx = get_context()
    f = np.array([p[0] for p in peaks], np.int64)
    t = np.array([p[1] for p in peaks], np.int64)
    if len(f) and (f.min() < 0 or f.max() > 4095 or t.min() < 0 or t.max() >= 2 ** 32):
        raise NotImplementedError("peak coordinates outside the packed-key range (freq < 4096)")
    k, t1, _ = ctx.pair_hash(f.astype(np.uint16), t.astype(np.uint32), np.array([0, len(f)], np.uint64), int(fan_value))
    return list(zip(hex_of_keys(ctx, k), t1.tolist()))


# ---- match / align (recognizer.py:222-338) -------------------------------------------------
def _result_dicts(db, res, q, queried_hashes):
    out = []
    for n in range(int(res["nres"][q])):
        song_id = int(res["sid"][q, n])
        song = db.get_song_by_id(song_id)
        offset = int(res["delta"][q, n])
        hashes_matched = int(res["dedup"][q, n])
        song_hashes = song.get(FIELD_TOTAL_HASHES, None)
        out.append({
            SONG_ID: song_id,
            SONG_NAME: song.get(SONG_NAME, None).encode("utf8"),
            INPUT_HASHES: queried_hashes,
            FINGERPRINTED_HASHES: song_hashes,
            HASHES_MATCHED: hashes_matched,
            INPUT_CONFIDENCE: round(hashes_matched / queried_hashes, 2),
            FINGERPRINTED_CONFIDENCE: round(hashes_matched / song_hashes, 2),
            OFFSET: offset,
            OFFSET_SECS: round(float(offset) / DEFAULT_FS * DEFAULT_WINDOW_SIZE * DEFAULT_OVERLAP_RATIO, 5),
            FIELD_FILE_SHA1: song.get(FIELD_FILE_SHA1, None).encode("utf8"),
        })
    return out


def _frames_secs(frames: int) -> float:
    return round(float(frames) / DEFAULT_FS * DEFAULT_WINDOW_SIZE * DEFAULT_OVERLAP_RATIO, 5)


def _add_extents(db, results, key32, q_off, query_off, res):
    """the extent keys of recognize_batch(extents=True), from one match_extents call on the results' (song, delta)"""
    from .extent import extents_of
    db.finalize()
    if not hasattr(db.table, "h"):
        raise NotImplementedError("extents take the unsharded table (shards=1)")
    ext = extents_of(db.table, key32, q_off, query_off, res, tol=db.ctx.vote_tolerance)
    for q, dicts in enumerate(results):
        for n, d in enumerate(dicts):
            qf, ql, tf, tl = (int(ext[f][q, n]) for f in ("q_first", "q_last", "t_first", "t_last"))
            d.update({"query_first": qf, "query_last": ql, "song_first": tf, "song_last": tl,
                      "query_start_secs": _frames_secs(qf), "query_end_secs": _frames_secs(ql + 1),
                      "song_start_secs": _frames_secs(tf), "song_end_secs": _frames_secs(tl + 1),
                      "extent_hist": ext["hist"][q, n].copy(), "extent_shift": int(ext["shift"][q])})


def _add_floor(results, res):
    """the "floor" entry of recognize_batch(floor=True): on the first result dict of every query that has one"""
    from .floor import floor_entry
    for q, dicts in enumerate(results):
        if dicts:
            dicts[0]["floor"] = floor_entry(res["song_hist"][q], res["bin_hist"][q], int(res["aligned"][q, 0]))


def _recognize_fused(queries, chans, owner, db, Fs, topn, resample_to=None, floor=False):
    """recognize_batch through shz_recognize_batch: one call, the hashes never leave the device."""
    if not hasattr(db.table, "h"):
        raise NotImplementedError("fused recognition takes the unsharded table (shards=1)")
    ctx = db.ctx
    if getattr(ctx, "hop", HOP) != HOP:
        ctx.set_overlap(NFFT - HOP)
    db.finalize()
    nq = len(queries)
    first = np.searchsorted(np.asarray(owner, np.int64), np.arange(nq + 1)).astype(np.uint32)

    def call(*a, **kw):     # floor: the rows the one call records, taken before the setting goes back
        with ctx.floor(floor):
            res, ms_extract, ms_match = ctx.recognize_batch(*a, **kw)
            if floor:
                res["song_hist"], res["bin_hist"] = ctx.take_floor()
                if len(res["song_hist"]) != nq:
                    raise RuntimeError(f"vote floor: {len(res['song_hist'])} rows recorded for {nq} queries")
        return res, ms_extract, ms_match

    if resample_to is not None and int(resample_to) != int(Fs):   # resampled on the device and handed on there
        buf, off = resample_to_device(chans, int(Fs), int(resample_to), ctx)
        try:
            res, ms_extract, ms_match = call(db.table, buf, off, first, fs=int(resample_to), amp_min=float(DEFAULT_AMP_MIN),
                                             fan_value=DEFAULT_FAN_VALUE, topn=int(topn), pcm_device=True)
        finally:
            buf.free()
    else:
        arrs = [_as_pcm(c) for c in chans]
        off = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)
        res, ms_extract, ms_match = call(db.table, pcm, off, first, fs=int(Fs), amp_min=float(DEFAULT_AMP_MIN),
                                         fan_value=DEFAULT_FAN_VALUE, topn=int(topn))
    t0 = time()
    results = [_result_dicts(db, res, q, int(res["nhash"][q])) for q in range(nq)]
    if floor:
        _add_floor(results, res)
    align_time = time() - t0
    return results, {"fingerprint_time": ms_extract * 1e-3, "query_time": ms_match * 1e-3, "align_time": align_time,
                     "n_matches": res["npairs"], "n_hashes": res["nhash"]}


@takes_key_cap(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
@takes_song_filter(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
@takes_delta_tol(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
def recognize_batch(queries, db, Fs: int = RATE, topn: int = TOPN, fused: bool = False, resample_to: int = None,
                    extents: bool = False, floor: bool = False):
    """Recognise flow (recognizer.py:377-392) for many queries at once.  Each query is a list of
    channels (1-D int16 arrays) or a single 1-D array.  Returns (results_per_query, timings).
    fused: fingerprint and match in ONE library call with the hashes staying on the device (shz_recognize_batch);
    same results, fingerprint_time / query_time are then the device times of the two halves.
    resample_to: the queries are at Fs, the table at resample_to (see fingerprint_batch); either path.
    delta_tol= (keyword): the vote tolerance in offset bins for this call (Context.tolerance); None: the context's.
    extents: every result dict also says WHERE the match holds (extent.extents_of at the call's tolerance): "query_first" /
    "query_last" / "song_first" / "song_last" (frames of the first and last aligned hash in the query and in the song),
    "query_start_secs" / "query_end_secs" / "song_start_secs" / "song_end_secs" (frames converted as "offset_seconds"
    converts, the end taken at last + 1), "extent_hist" (64 counts over the query's time) and "extent_shift" (bucket b of
    it covers the query frames [b << shift, (b + 1) << shift)).  Not with fused: that call keeps its hashes inside the
    library.
    floor: the first result dict of every query gains "floor": {"song_hist", "bin_hist"} -- the query's two vote-floor
    histograms ([32] uint32, Context.floor) -- and {"expected_above", "score"} -- what shazam_amd.floor.expected_above / score
    make of song_hist and the query's best aligned count (a heuristic; None where nothing can be fitted).  The other entries
    do not change; either path, with resample_to and delta_tol.
    songs= / exclude= (keywords, song ids): the queries are matched within / without these songs (Context.songs,
    Table.match(songs=)): the results of the same call on a database holding only the allowed songs, "n_matches" counting
    the kept pairs; either path; the unsharded table only (a sharded database: NotImplementedError).
    max_key_rows= (keyword): the key cap of this call (Context.key_cap: keys that hold more table rows vote for nobody;
    shazam_amd.keycap.cap_for picks one from Table.key_hist()); either path, sharded or not; with extents, the extents cover
    the kept pairs.  None: the context's.  recognize_speeds / recognize_warps, find_duplicates / match_songs, the listeners
    and match_extents have no such keyword: run them inside `with ctx.key_cap(rows):`."""
    if extents and fused:
        raise ValueError("extents=True needs the query's hashes on the host: not with fused=True")
    ctx = db.ctx
    chans, owner = [], []
    for qi, q in enumerate(queries):
        cs = [q] if (isinstance(q, np.ndarray) and q.ndim == 1) else list(q)
        chans.extend(cs)
        owner.extend([qi] * len(cs))
    if fused:
        return _recognize_fused(queries, chans, owner, db, Fs, topn, resample_to, floor)
    t0 = time()
    k, t1, ho = fingerprint_batch(chans, Fs, ctx=ctx, resample_to=resample_to)
    fingerprint_time = time() - t0
    # channels of one query are adjacent, so the per-query CSR is a sub-sampling of hash_off
    owner = np.asarray(owner, np.int64)
    nq = len(queries)
    first = np.searchsorted(owner, np.arange(nq + 1))
    qoff = ho[first]
    t0 = time()
    res = db.match(k, t1, qoff, topn, floor=floor)
    query_time = time() - t0
    t0 = time()
    results = [_result_dicts(db, res, q, int(res["nhash"][q])) for q in range(nq)]
    if floor:
        _add_floor(results, res)
    if extents:
        _add_extents(db, results, k, t1, qoff, res)
    align_time = time() - t0
    return results, {"fingerprint_time": fingerprint_time, "query_time": query_time, "align_time": align_time,
                     "n_matches": res["npairs"], "n_hashes": res["nhash"]}


def recognize(channels_or_samples, db=None, Fs: int = RATE, topn: int = TOPN, fused: bool = False, resample_to: int = None,
              delta_tol: int = None, extents: bool = False, floor: bool = False, songs=None, exclude=None, max_key_rows=None):
    """recognizer.py:377-396: (final_results, fingerprint_time, query_time, align_time).  fused, resample_to, delta_tol,
    extents, floor, songs, exclude, max_key_rows: see recognize_batch."""
    if db is None:
        raise ValueError("recognize() needs the HipFingerprintDB holding the fingerprints")
    x = channels_or_samples
    q = [np.asarray(x)] if (not isinstance(x, (list, tuple)) or (len(x) and np.isscalar(x[0]))) else list(x)
    results, tm = recognize_batch([q], db, Fs, topn, fused, resample_to, extents, floor, delta_tol=delta_tol, songs=songs,
                                  exclude=exclude, max_key_rows=max_key_rows)
    return results[0], tm["fingerprint_time"], tm["query_time"], tm["align_time"]


# live streams (recognizer.py:21-25, 357-392): incremental fingerprints and recognition of chunked input
from .stream import StreamFingerprinter, StreamRecognizer, fingerprint_stream  # noqa: E402,F401
# sample-rate conversion (csrc/shz_resample.hip): audio at any rate against a table at another
from .resample import StreamResampler, resample_batch, resample_plan, resample_to_device  # noqa: E402,F401
# long recordings (csrc/shz_scan.hip): every window of a recording matched in one call, and the timeline of its songs
from .scan import scan, scan_windows  # noqa: E402,F401
# queries played fast or slow (csrc/shz_speed.hip): the peaks warped for every factor of a ladder, all variants in one match
from .speed import (pitch_ladder, recognize_speeds, recognize_warps, speed_ladder, tempo_ladder, warp_grid,  # noqa: E402,F401
                    warp_hashes, warp_hashes_tf)
# the key cap's arithmetic on a table's key-size histogram (Table.key_hist)
from . import keycap  # noqa: E402,F401
# the catalogue against itself (csrc/shz_catalog.hip): the rows of listed songs as queries, duplicates and excerpts among them
from .catalog import find_duplicates, fold_pairs, fold_pairs_warps, match_songs  # noqa: E402,F401
# repeated content inside recordings, no catalogue (csrc/shz_repeat.hip): the lag histogram of a recording against itself
from .repeats import find_repeats, find_repeats_hashes, occurrences  # noqa: E402,F401
# content shared between recordings, no catalogue (csrc/shz_repeat.hip, the job form): a signed lag histogram per pair of recordings
from .shared import cells_fit, find_shared, find_shared_hashes, find_shared_peaks, shared_occurrences  # noqa: E402,F401
