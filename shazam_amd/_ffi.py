"""ctypes binding of libshz.so (include/shz.h).  numpy + ctypes only -- no torch, no CPU fallback:
if the HIP library is missing or a call fails this module raises."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SHZ_LIB") or os.path.join(_HERE, "libshz.so")  # SHZ_LIB: A/B builds of the same ABI

OK, E_INVALID, E_HIP, E_CAPACITY, E_NOMEM, E_UNSUPPORTED, E_RCCL, E_STATE = 0, -1, -2, -3, -4, -5, -6, -7
PCM_DEVICE, OUT_DEVICE, IN_DEVICE, STFT_POWER, MATCH_FULL_SORT, RESERVE_GATHER, RESERVE_WAIT = 1, 2, 4, 8, 16, 32, 64
SCAN_KEEP_MASK = 128   # shz_scan_extents: out_nres holds a keep mask of the windows on entry
SONGS_DEVICE_OUT = 128   # shz_table_song_hashes: key32 / off are device memory
# shz_set_debug test switches (include/shz.h); RUN_ROWS_MAX[_SMALL]: the most rows a run / a segment cut from runs holds
DEBUG_VT_TINY_HEAVY, DEBUG_VT_PROBE1, DEBUG_RUN_LIMIT_SMALL, DEBUG_SCAN_SMALL_GROUPS = 1, 2, 4, 8
DEBUG_SPEED_SMALL_SLICES = 16   # shz_recognize_speeds: at most 2 queries a slice
DEBUG_SCAN_SPEED_SMALL_SLICES = 32   # shz_scan_speeds: at most 1 recording x 2 rungs a slice, 3 windows a match group
DEBUG_CATALOG_SMALL_SLICES = 64   # shz_match_songs_warps: one song x at most 2 warps a slice
DEBUG_VOTE_TOLERANT_ROUTE = 128   # the vote: the tolerant route at tolerance 0 too
DEBUG_EXTENT_SMALL_TILES = 256   # shz_match_extents: tiles of 64 pairs, 4 descriptors in LDS, 3 queries a sub-batch
DEBUG_REPEAT_SMALL_SLICES = 512  # shz_repeats_* / shz_shared_*: one recording (job) a slice, expand tiles of 64 pairs, blocks of 64 elements
DEBUG_FLOOR_SMALL = 1024         # the vote floor: at most 3 queries a match sub-batch, 2 queries in the histogram kernels' LDS table
DEBUG_FILTER_SMALL = 2048        # the song filter: filter kernels' blocks of 64 votes, at most 3 queries a match sub-batch
FILTER_EXCLUDE = 1               # shz_set_song_filter: the listed songs are barred (SHZ_FILTER_EXCLUDE)
SHARED_LAG_BIAS = 1 << 20        # shz_shared_*: cell_lag = lag + SHARED_LAG_BIAS (SHZ_SHARED_LAG_BIAS)
SCAN_NO_WARP = 0xFFFFFFFF            # shz_scan_warps: out_best of a window that tried no variant
SCAN_U32, SCAN_POPC64, SCAN_U64 = 0, 1, 2   # shz_scan_host kinds
STAGE_F32, STAGE_F64, STAGE_PERSISTENT = 0, 1, 1   # shz_stft_stage_host kinds | flag
RUN_ROWS_MAX, RUN_ROWS_MAX_SMALL = (1 << 32) - 4096, 65536
NFFT, HOP, NBINS = 4096, 2048, 2049

u8p, u16p, u32p, i32p, u64p, i16p, f64p = (C.POINTER(t) for t in (
    C.c_uint8, C.c_uint16, C.c_uint32, C.c_int32, C.c_uint64, C.c_int16, C.c_double))
vp = C.c_void_p

# name -> (restype, argtypes); the loader test checks every symbol in include/shz.h is exported
SIGNATURES = {
    "shz_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(vp)]),
    "shz_ctx_destroy": (C.c_int32, [vp]),
    "shz_last_error": (C.c_char_p, [vp]),
    "shz_version": (C.c_char_p, []),
    "shz_device_info": (C.c_int32, [vp, C.c_char_p, C.c_uint64, u64p, i32p, i32p]),
    "shz_mem_info": (C.c_int32, [vp, u64p, u64p]),
    "shz_dev_alloc": (C.c_int32, [vp, C.c_uint64, C.POINTER(vp)]),
    "shz_dev_free": (C.c_int32, [vp, vp]),
    "shz_copy_h2d": (C.c_int32, [vp, vp, vp, C.c_uint64]),
    "shz_copy_d2h": (C.c_int32, [vp, vp, vp, C.c_uint64]),
    "shz_sync": (C.c_int32, [vp]),
    "shz_host_alloc": (C.c_int32, [vp, C.c_uint64, C.POINTER(vp)]),
    "shz_host_free": (C.c_int32, [vp, vp]),
    "shz_set_workspace_limit": (C.c_int32, [vp, C.c_uint64]),
    "shz_release_workspace": (C.c_int32, [vp, u64p]),
    "shz_timer_start": (C.c_int32, [vp, C.c_int32]),
    "shz_timer_stop": (C.c_int32, [vp, C.c_int32, C.POINTER(C.c_float)]),
    "shz_set_profiling": (C.c_int32, [vp, C.c_int32]),
    "shz_get_kernel_ms": (C.c_int32, [vp, C.c_int32, C.POINTER(C.c_float), u32p]),
    "shz_synth_pcm": (C.c_int32, [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.c_uint64, vp]),
    "shz_synth_corpus": (C.c_int32, [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_uint64, vp]),
    "shz_sumsq_i16": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint64, u64p]),
    "shz_mix_i16": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint64, f64p, vp]),
    "shz_membw": (C.c_int32, [vp, C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(C.c_float)]),
    "shz_sort_pairs": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]),
    "shz_sort_keys32": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, vp]),
    "shz_sort_keys32_seg": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "shz_scan_host": (C.c_int32, [vp, C.c_uint32, vp, vp, C.c_uint64, C.c_uint32, u64p]),
    "shz_frame_count": (C.c_uint32, [C.c_uint64]),
    "shz_frame_count_hop": (C.c_uint32, [C.c_uint64, C.c_uint32]),
    "shz_set_overlap": (C.c_int32, [vp, C.c_uint32]),
    "shz_numpy_tables": (C.c_int32, [C.c_uint32, vp, vp, vp]),
    "shz_set_numpy_window": (C.c_int32, [vp, vp, C.c_double]),
    "shz_set_numpy_product": (C.c_int32, [vp, C.c_int32]),
    "shz_stft_db_any": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p]),
    "shz_stft_db": (C.c_int32, [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p]),
    "shz_stft_stage_host": (C.c_int32, [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p]),
    "shz_db_values": (C.c_int32, [vp, C.c_uint64, vp]),
    "shz_peaks": (C.c_int32, [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, vp, vp, u64p, C.c_uint64, u64p]),
    "shz_peaks_from_db": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_double, vp, vp, C.c_uint64, u64p]),
    "shz_pair_hash": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, C.c_uint32, vp, vp, u64p, C.c_uint64, u64p]),
    "shz_fingerprint_batch": (C.c_int32, [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32,
                                          vp, vp, u64p, C.c_uint64, u64p]),
    "shz_set_stage_f64": (C.c_int32, [vp, C.c_int32]),
    "shz_set_vote_tolerance": (C.c_int32, [vp, C.c_uint32]),
    "shz_get_vote_tolerance": (C.c_int32, [vp, u32p]),
    "shz_set_vote_floor": (C.c_int32, [vp, C.c_uint32]),
    "shz_get_vote_floor": (C.c_int32, [vp, u32p]),
    "shz_set_song_filter": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32]),
    "shz_get_song_filter": (C.c_int32, [vp, u32p, u32p, u64p]),
    "shz_match_batch_sets": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "shz_match_device_host_sets": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64, vp, vp, vp, vp,
                                               vp, vp, vp, vp]),
    "shz_vote_floor_rows": (C.c_int32, [vp, u64p]),
    "shz_vote_floor_take": (C.c_int32, [vp, vp, vp, C.c_uint64, u64p]),
    "shz_vote_bucket": (C.c_int32, [C.c_uint32, u32p]),
    "shz_upload_stats": (C.c_int32, [vp, u64p, u64p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "shz_extract_stats": (C.c_int32, [vp, u64p, u64p, u64p, u64p, u64p, u64p]),
    "shz_sha1_prefix": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint32, vp]),
    "shz_sha1_invert": (C.c_int32, [vp, vp, C.c_uint64, vp]),
    "shz_table_create": (C.c_int32, [vp, C.POINTER(vp)]),
    "shz_table_destroy": (C.c_int32, [vp]),
    "shz_table_insert": (C.c_int32, [vp, vp, vp, vp, C.c_uint64, C.c_uint32]),
    "shz_table_insert_clips": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "shz_table_finalize": (C.c_int32, [vp]),
    "shz_table_set_segment_rows": (C.c_int32, [vp, C.c_uint64]),
    "shz_table_reserve": (C.c_int32, [vp, C.c_uint64, C.c_uint64, C.c_uint32]),
    "shz_table_seal_run": (C.c_int32, [vp]),
    "shz_table_rows": (C.c_int32, [vp, u64p, u64p]),
    "shz_table_segments": (C.c_int32, [vp, vp]),
    "shz_table_delete_songs": (C.c_int32, [vp, vp, C.c_uint64, u64p]),
    "shz_table_clear": (C.c_int32, [vp]),
    "shz_table_export": (C.c_int32, [vp, vp, vp, vp, C.c_uint64, u64p]),
    "shz_table_lookup": (C.c_int32, [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, u64p]),
    "shz_table_song_rows": (C.c_int32, [vp, C.c_uint32, u64p]),
    "shz_table_song_hashes": (C.c_int32, [vp, vp, C.c_uint32, u64p, vp, vp, C.c_uint64, C.c_uint32]),
    "shz_match_songs": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "shz_match_extents": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "shz_match_extents_fit": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp, vp]),
    "shz_match_songs_extents": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "shz_warp_row_host": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp]),
    "shz_warp_rows": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, vp, vp, u64p, C.c_uint64,
                                  u64p]),
    "shz_match_songs_warps": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, vp, vp, vp, vp,
                                          vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_match_songs_warps_extents": (C.c_int32, [vp, vp, u32p, u32p, u32p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                  vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_float)]),
    "shz_match_batch": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32,
                                    vp, vp, vp, vp, vp, vp, vp]),
    "shz_match_device_host": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64,
                                          vp, vp, vp, vp, vp, vp, vp]),
    "shz_recognize_batch": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                        C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float),
                                        C.POINTER(C.c_float)]),
    "shz_recognize_estimate": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "shz_match_stats": (C.c_int32, [vp, u64p, u64p, u64p]),
    "shz_set_debug": (C.c_int32, [vp, C.c_uint32]),
    "shz_set_key_cap": (C.c_int32, [vp, C.c_uint64]),
    "shz_get_key_cap": (C.c_int32, [vp, u64p]),
    "shz_key_cap_stats": (C.c_int32, [vp, u64p, u64p]),
    "shz_table_key_hist": (C.c_int32, [vp, vp, vp, u64p, u64p]),
    "shz_match_vt_redo": (C.c_int32, [vp, u64p]),
    "shz_match_spec_stats": (C.c_int32, [vp, u64p, u64p]),
    "shz_comm_unique_id": (C.c_int32, [vp]),
    "shz_comm_create": (C.c_int32, [vp, vp, C.c_int32, C.c_int32, C.POINTER(vp)]),
    "shz_comm_create_local": (C.c_int32, [vp, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(vp)]),
    "shz_comm_destroy": (C.c_int32, [vp]),
    "shz_table_allgather": (C.c_int32, [vp, vp, u64p]),
    "shz_table_exchange_run": (C.c_int32, [vp, vp]),
    "shz_table_exchange_stats": (C.c_int32, [vp, u64p, u64p, C.POINTER(C.c_double), u32p]),
    "shz_table_set_run_rows": (C.c_int32, [vp, C.c_uint64]),
    "shz_table_finalize_runs": (C.c_int32, [vp, u64p, C.c_uint32]),
    "shz_table_build_stats": (C.c_int32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]),
    "shz_table_phase_stats": (C.c_int32, [vp, C.POINTER(C.c_double), C.c_uint32, u32p, C.c_int32]),
    "shz_table_phase_name": (C.c_char_p, [C.c_uint32]),
    "shz_comm_barrier": (C.c_int32, [vp]),
    "shz_comm_warmup": (C.c_int32, [vp]),
    "shz_shard_of_keys": (C.c_int32, [vp, C.c_uint64, C.c_uint32, vp]),
    "shz_table_keep_shard": (C.c_int32, [vp, C.c_uint32, C.c_uint32]),
    "shz_table_shard_exchange": (C.c_int32, [vp, vp, u64p]),
    "shz_table_stage_from": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32]),
    "shz_table_clear_staged": (C.c_int32, [vp]),
    "shz_table_maxima": (C.c_int32, [vp, u32p, u32p]),
    "shz_match_pairs": (C.c_int32, [vp, vp, vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p, vp, vp]),
    "shz_pairs_allgather": (C.c_int32, [vp, C.c_uint64, vp, vp, C.c_uint64, u64p]),
    "shz_pairs_vote": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   vp, vp, vp, vp, vp]),
    "shz_streams_create": (C.c_int32, [vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(vp)]),
    "shz_streams_destroy": (C.c_int32, [vp]),
    "shz_streams_push": (C.c_int32, [vp, vp, u64p, vp, C.c_uint32, vp, vp, u64p, C.c_uint64, u64p]),
    "shz_streams_reset": (C.c_int32, [vp, vp, C.c_uint32]),
    "shz_streams_state": (C.c_int32, [vp, C.c_uint32, u64p, u64p, u64p, u64p]),
    "shz_stream_plan": (C.c_int32, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, u64p, u64p, u64p, u64p]),
    "shz_listeners_create": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "shz_listeners_destroy": (C.c_int32, [vp]),
    "shz_listeners_push": (C.c_int32, [vp, vp, u64p, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "shz_listeners_reset": (C.c_int32, [vp, vp, C.c_uint32]),
    "shz_listeners_state": (C.c_int32, [vp, C.c_uint32, u64p, u64p]),
    "shz_listeners_window": (C.c_int32, [vp, C.c_uint32, vp, vp, vp, C.c_uint64, u64p]),
    "shz_listeners_create_peaks": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "shz_listeners_push_warps": (C.c_int32, [vp, vp, u64p, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp,
                                             vp, vp]),
    "shz_listeners_push_speeds": (C.c_int32, [vp, vp, u64p, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp]),
    "shz_listeners_peaks": (C.c_int32, [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, u64p]),
    "shz_listeners_timing": (C.c_int32, [vp, C.c_int32, vp]),
    "shz_listener_window": (C.c_int32, [u64p, C.c_uint32, C.c_uint32, u64p, u64p]),
    "shz_resample_i16": (C.c_int32, [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32,
                                     vp, u64p, C.c_uint64, u64p]),
    "shz_scan_window_count": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "shz_scan_batch": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, vp, vp, vp, vp, vp, vp, vp, C.c_uint64,
                                   u64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_scan_timeline": (C.c_int32, [u64p, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p]),
    "shz_scan_zones": (C.c_int32, [vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]),
    "shz_scan_extents": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     u64p, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p,
                                     vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_warp_pair_hash":(C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                       vp, vp, u64p, C.c_uint64, u64p]),
    "shz_recognize_speeds": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                         C.c_uint32, u32p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                         C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_recognize_speeds_extents": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                                 C.c_uint32, u32p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                 C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32,
                                                 vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]),
    "shz_warp_pair_hash_tf": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32,
                                          C.c_uint32, vp, vp, u64p, C.c_uint64, u64p]),
    "shz_recognize_warps": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                        C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_recognize_warps_extents": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                                C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32,
                                                vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]),
    "shz_scan_speeds": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u64p, vp, vp, vp, vp, vp, vp,
                                    vp, vp, vp, C.c_uint64, u64p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_scan_timeline_speeds": (C.c_int32, [u64p, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, u32p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                             C.c_uint64, u64p]),
    "shz_scan_warps": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, u64p, vp, vp,
                                   vp, vp, vp, vp, vp, vp, vp, u64p, C.c_uint64, u64p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_scan_timeline_warps": (C.c_int32, [u64p, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp,
                                            vp, vp, C.c_uint64, u64p]),
    "shz_scan_play_zones": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
    "shz_scan_plays": (C.c_int32, [vp, vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                   vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_repeats_hashes": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p]),
    "shz_repeats_batch": (C.c_int32, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                      vp, C.c_uint64, u64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_repeats_fold": (C.c_int32, [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp,
                                     vp, vp, C.c_uint64, u64p]),
    "shz_shared_hashes": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p]),
    "shz_shared_batch": (C.c_int32, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, vp, vp, C.c_uint32,
                                     C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                     vp, vp, C.c_uint64, u64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "shz_shared_warps_peaks": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp, vp,
                                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp,
                                           vp, vp, vp, C.c_uint64, u64p]),
    "shz_shared_warps_batch": (C.c_int32, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, vp, vp, C.c_uint32,
                                           vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                           C.POINTER(C.c_float), C.POINTER(C.c_float)]),
}


_NP_FUSED = None


def numpy_product_is_fused() -> bool:
    """Does this host's numpy form the real part of conj(z) * z as fma(re, re, im * im)?  (mlab's `np.conj(result) * result`;
    numpy's SIMD complex product uses FMA3 where the CPU has it.)  Probed once on values for which the two roundings differ;
    an inconclusive probe means fused, the form of the hosts that made the fixtures."""
    global _NP_FUSED
    if _NP_FUSED is None:
        import fractions
        rng = np.random.default_rng(12345)
        z = (rng.standard_normal(64) + 1j * rng.standard_normal(64)) * 1e3
        got = (np.conj(z) * z).real
        votes = []
        for v, g in zip(z, got):
            re, im = float(v.real), float(v.imag)
            plain = re * re + im * im
            exact = fractions.Fraction(re) * fractions.Fraction(re) + fractions.Fraction(im * im)   # what an FMA rounds
            fused = float(exact)                                                                   # (Fraction -> float rounds to nearest even)
            if plain != fused:
                votes.append(g == fused)
        _NP_FUSED = bool(sum(votes) * 2 >= len(votes)) if votes else True
    return _NP_FUSED


def takes_delta_tol(ctx_of):
    """Decorator: the function gains the keyword delta_tol=None -- the vote tolerance in offset bins that holds while it runs
    (Context.tolerance; None: the context stays as it is).  ctx_of(*args, **kw) finds the Context among its arguments."""
    def deco(fn):
        @functools.wraps(fn)
        def run(*args, delta_tol=None, **kw):
            if delta_tol is None:
                return fn(*args, **kw)
            with ctx_of(*args, **kw).tolerance(delta_tol):
                return fn(*args, **kw)
        return run
    return deco


def _song_ids(a):
    """any iterable of song ids -> a contiguous uint32 array"""
    v = np.asarray(a if isinstance(a, np.ndarray) else sorted(a) if isinstance(a, (set, frozenset)) else list(a))
    if v.size and (v.min() < 0 or v.max() >= 1 << 32):
        raise ValueError("song ids must fit 32 bits")
    return np.ascontiguousarray(v.reshape(-1), np.uint32)


def _song_sets(sets):
    """one iterable of ids, or a list of iterables -> a list of uint32 arrays (a sequence whose entries are all iterable is
    a list of sets; an empty one is ONE empty set)"""
    if isinstance(sets, np.ndarray) and sets.ndim <= 1:
        return [_song_ids(sets)]
    sets = list(sets)
    if sets and all(hasattr(a, "__iter__") for a in sets):
        return [_song_ids(a) for a in sets]
    return [_song_ids(sets)]


def takes_song_filter(ctx_of):
    """Decorator: the function gains the keywords songs=None and exclude=None -- song ids the call matches within / without
    (Context.songs: the song filter while it runs, the previous one afterwards; both None: the context stays as it is; both
    given: ValueError).  The library-internal queries of the call (windows, variants) all use the one set.  ctx_of(*args,
    **kw) finds the Context among its arguments."""
    def deco(fn):
        @functools.wraps(fn)
        def run(*args, songs=None, exclude=None, **kw):
            if songs is None and exclude is None:
                return fn(*args, **kw)
            with ctx_of(*args, **kw).songs(only=songs, exclude=exclude):
                return fn(*args, **kw)
        return run
    return deco


def takes_key_cap(ctx_of):
    """Decorator: the function gains the keyword max_key_rows=None -- the key cap that holds while it runs (Context.key_cap:
    keys that hold more table rows vote for nobody; 0: off; None: the context stays as it is).  ctx_of(*args, **kw) finds the
    Context among its arguments."""
    def deco(fn):
        @functools.wraps(fn)
        def run(*args, max_key_rows=None, **kw):
            if max_key_rows is None:
                return fn(*args, **kw)
            with ctx_of(*args, **kw).key_cap(max_key_rows):
                return fn(*args, **kw)
        return run
    return deco


class _KeyCap(int):
    """Context.key_cap: the cap in force as an int, and -- called with a cap -- the block that sets it for a while."""

    def __new__(cls, ctx, rows):
        self = super().__new__(cls, rows)
        self._ctx = ctx
        return self

    @contextlib.contextmanager
    def __call__(self, rows):
        ctx = self._ctx
        if rows is None:
            yield ctx
            return
        before = int(ctx.key_cap)
        ctx.set_key_cap(rows)
        try:
            yield ctx
        finally:
            ctx.set_key_cap(before)


class ShzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libshz error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libshz.so (built in-tree by __graft_entry__.build() / make -C shazam_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `make -C shazam_amd/csrc` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def ptr(a):
    """void* of a numpy array (or pass through ints / None)."""
    if a is None:
        return None
    if isinstance(a, (int,)):
        return C.c_void_p(a)
    if isinstance(a, DevBuf):
        return C.c_void_p(a.ptr)
    return C.c_void_p(a.ctypes.data)


class DevBuf:
    """Caller-owned device allocation (shz_dev_alloc)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = vp()
        ctx.check(lib().shz_dev_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr and self.ctx.h:
            self.ctx.check(lib().shz_dev_free(self.ctx.h, vp(self.ptr)))
        self.ptr = None

    def upload(self, arr: np.ndarray, offset_bytes: int = 0):
        arr = np.ascontiguousarray(arr)
        assert offset_bytes + arr.nbytes <= self.nbytes
        self.ctx.check(lib().shz_copy_h2d(self.ctx.h, vp(self.ptr + offset_bytes), ptr(arr), arr.nbytes))

    def download(self, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        out = np.empty(count, dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        self.ctx.check(lib().shz_copy_d2h(self.ctx.h, ptr(out), vp(self.ptr + offset_bytes), out.nbytes))
        return out

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One (device, stream).  Not thread-safe; use one per thread/process."""

    def __init__(self, device_id: int = 0):
        self.h = None
        h = vp()
        rc = lib().shz_ctx_create(device_id, C.byref(h))
        if rc != OK:
            raise ShzError(rc, f"shz_ctx_create(device {device_id}) failed -- is a ROCm GPU visible?")
        self.h = h
        self.device_id = device_id
        # the fp64 path's window as THIS host's numpy forms it (mlab.window_hanning = np.hanning; the scaling by
        # (window ** 2).sum()): numpy's by construction, not by the agreement of two cosine routines
        w = np.hanning(4096)
        self.check(lib().shz_set_numpy_window(self.h, ptr(w), float((w ** 2).sum())))
        self.check(lib().shz_set_numpy_product(self.h, 1 if numpy_product_is_fused() else 0))

    def check(self, rc):
        if rc != OK:
            raise ShzError(rc, (lib().shz_last_error(self.h) or b"").decode(errors="replace"))

    def close(self):
        if self.h:
            lib().shz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- info / memory -------------------------------------------------------------------
    def device_info(self):
        name = C.create_string_buffer(256)
        hbm, cus, clk = C.c_uint64(), C.c_int32(), C.c_int32()
        self.check(lib().shz_device_info(self.h, name, 256, C.byref(hbm), C.byref(cus), C.byref(clk)))
        return {"name": name.value.decode(), "hbm_bytes": hbm.value, "compute_units": cus.value, "clock_khz": clk.value}

    def set_debug(self, flags: int):
        """SHZ_DEBUG_* test switches (1: tiny hand-over list, 2: LDS probes give up after one round, 4: runs and segments cut
        from runs hold at most RUN_ROWS_MAX_SMALL rows, 8: shz_scan_batch matches its windows in groups of at most 3, 16: shz_recognize_speeds warps and
        matches its queries in slices of at most 2, 32: shz_scan_speeds works in slices of 1 recording x 2 rungs and matches
        its windows in groups of at most 3, 64: shz_match_songs_warps works in slices of 1 song x 2 warps, 128: the vote takes
        the tolerant route at tolerance 0 too, 256: the extent kernel works in tiles of 64 pairs with 4 descriptors in LDS and
        sub-batches of 3 queries, 512: shz_repeats_* works in slices of one recording, expand tiles of 64 pairs and blocks of
        64 elements, 1024: with the vote floor on, match sub-batches of at most 3 queries and histogram kernels with 2
        queries in LDS, 2048: with a song filter set, filter kernels whose blocks hold 64 votes and match sub-batches of at
        most 3 queries)."""
        self.check(lib().shz_set_debug(self.h, int(flags)))

    def set_vote_tolerance(self, bins: int):
        """Every later vote of this context sums a song's aligned count over bins + 1 neighbouring offset bins
        (shz_set_vote_tolerance; 0: one bin, the default; more than 31: ShzError, the setting stays)."""
        if not 0 <= int(bins) < 1 << 32:
            raise ShzError(E_INVALID, f"vote tolerance {bins}")
        self.check(lib().shz_set_vote_tolerance(self.h, int(bins)))

    @property
    def vote_tolerance(self) -> int:
        n = C.c_uint32()
        self.check(lib().shz_get_vote_tolerance(self.h, C.byref(n)))
        return n.value

    @contextlib.contextmanager
    def tolerance(self, bins):
        """with ctx.tolerance(bins): the vote tolerance inside the block, the previous one after it (also after an
        exception).  bins None: the context stays as it is."""
        if bins is None:
            yield self
            return
        before = self.vote_tolerance
        self.set_vote_tolerance(bins)
        try:
            yield self
        finally:
            self.set_vote_tolerance(before)

    # ---- the key cap (shz_set_key_cap) -----------------------------------------------------
    def set_key_cap(self, rows: int):
        """Every later match of this context leaves out the keys that hold more than `rows` table rows, counted over all
        segments (shz_set_key_cap): the result arrays are those of the plain match on a table lacking those keys' rows.
        0: off, the default.  A key with exactly `rows` rows stays.  Decided at the probe, so a dropped key costs neither
        expand, sort nor fold; the sharded table applies it exactly (a key lives on one shard)."""
        if not 0 <= int(rows) < 1 << 64:
            raise ShzError(E_INVALID, f"key cap {rows}")
        self.check(lib().shz_set_key_cap(self.h, int(rows)))

    @property
    def key_cap(self):
        """The key cap in force (an int; 0: off).  with ctx.key_cap(rows): the cap inside the block, the previous one after
        it (also after an exception; blocks nest).  rows None: the context stays as it is.  Every call that matches inside
        the block follows it: recognize_speeds / recognize_warps, find_duplicates / match_songs, the listeners,
        match_extents and the scans included."""
        n = C.c_uint64()
        self.check(lib().shz_get_key_cap(self.h, C.byref(n)))
        return _KeyCap(self, n.value)

    def key_cap_stats(self) -> dict:
        """{"groups", "pairs"}: the (query, key) groups and the pairs the key cap dropped in the last match call (0 with the
        cap off)."""
        g, p = C.c_uint64(), C.c_uint64()
        self.check(lib().shz_key_cap_stats(self.h, C.byref(g), C.byref(p)))
        return {"groups": g.value, "pairs": p.value}

    # ---- the vote floor (shz_set_vote_floor) ----------------------------------------------
    def set_vote_floor(self, on: bool):
        """Every later vote of this context records, per query, a row of two histograms: how many songs reached which best
        count and how many single bins reached which count (32 buckets, shazam_amd.floor.bucket_of).  A row costs 256 bytes
        of host memory until it is taken (take_floor); switching off drops the rows not taken."""
        self.check(lib().shz_set_vote_floor(self.h, 1 if on else 0))

    @property
    def vote_floor(self) -> bool:
        n = C.c_uint32()
        self.check(lib().shz_get_vote_floor(self.h, C.byref(n)))
        return bool(n.value)

    def floor_rows(self) -> int:
        """Rows recorded since the last take_floor()."""
        n = C.c_uint64()
        self.check(lib().shz_vote_floor_rows(self.h, C.byref(n)))
        return n.value

    def take_floor(self):
        """(song_hist, bin_hist), [n, 32] uint32 each: the rows recorded since the last take, in the order the queries were
        handed to the vote; the store is empty afterwards."""
        n = self.floor_rows()
        sh, bh = np.zeros((n, 32), np.uint32), np.zeros((n, 32), np.uint32)
        got = C.c_uint64()
        self.check(lib().shz_vote_floor_take(self.h, ptr(sh) if n else None, ptr(bh) if n else None, n, C.byref(got)))
        return sh, bh

    @contextlib.contextmanager
    def floor(self, on=True):
        """with ctx.floor(): the vote floor on inside the block; the previous state after it, and no rows left over from the
        block (also after an exception).  on False / None: the context stays as it is.  Where the floor was on already, the
        rows recorded before the block and not yet taken are dropped too (the store is one list: a call that asks for its own
        rows takes it whole) -- take_floor() first if they matter.  The same holds for floor=True on match(), recognize*() and
        scan_windows(), which run inside this block."""
        if not on:
            yield self
            return
        before = self.vote_floor
        self.set_vote_floor(True)
        try:
            yield self
        finally:
            self.set_vote_floor(False)      # drops the leftovers
            if before:
                self.set_vote_floor(True)

    # ---- the song filter (shz_set_song_filter) ---------------------------------------------
    def set_song_filter(self, sets, exclude=False):
        """Every later match of this context votes within a set of songs (shz_set_song_filter): the result arrays are those
        of the plain match on a table holding only the allowed songs' rows.  sets: one iterable of song ids, or a list of
        iterables (several sets: Table.match(song_sets=, set_of=) says which query uses which; every other call uses set
        0).  exclude: the listed songs are the barred ones.  An empty set allows nothing (exclude: bars nothing).  Ids in
        any order, repeats allowed.  The unsharded table only.  A refused call leaves the previous filter in force."""
        lists = _song_sets(sets)
        off = np.zeros(len(lists) + 1, np.uint64)
        off[1:] = np.cumsum([len(a) for a in lists], dtype=np.uint64)
        ids = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, np.uint32), np.uint32)
        self.check(lib().shz_set_song_filter(self.h, ptr(ids), ptr(off), len(lists), FILTER_EXCLUDE if exclude else 0))
        self._song_filter = (lists, bool(exclude)) if lists else None

    def clear_song_filter(self):
        """No song filter (the default): every song of the table is matched."""
        self.check(lib().shz_set_song_filter(self.h, None, None, 0, 0))
        self._song_filter = None

    @property
    def song_filter(self):
        """None, or {"n_sets", "exclude", "n_ids"} of the filter in force (shz_get_song_filter)."""
        n, f, ids = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.check(lib().shz_get_song_filter(self.h, C.byref(n), C.byref(f), C.byref(ids)))
        if n.value == 0:
            return None
        return {"n_sets": n.value, "exclude": bool(f.value & FILTER_EXCLUDE), "n_ids": ids.value}

    @contextlib.contextmanager
    def songs(self, only=None, exclude=None, sets=None):
        """with ctx.songs(only=ids) / ctx.songs(exclude=ids) / ctx.songs(sets=[ids, ...]): the song filter inside the block,
        the previous one after it (also after an exception; the wrapper keeps the lists it last sent).  With sets=,
        exclude=True makes every set a list of barred songs.  All three None: the context stays as it is.  only= together
        with an exclude= list, or with sets=: ValueError."""
        deny_list = exclude is not None and not isinstance(exclude, (bool, np.bool_))
        if only is not None and (deny_list or sets is not None):
            raise ValueError("songs(): only= goes without exclude= and without sets=")
        if sets is not None and deny_list:
            raise ValueError("songs(): with sets=, exclude is True or False")
        if only is None and sets is None and not deny_list:
            yield self
            return
        before = getattr(self, "_song_filter", None)
        if sets is not None:
            self.set_song_filter([_song_ids(a) for a in sets], exclude=bool(exclude))
        elif only is not None:
            self.set_song_filter([_song_ids(only)])
        else:
            self.set_song_filter([_song_ids(exclude)], exclude=True)
        try:
            yield self
        finally:
            if before is None:
                self.clear_song_filter()
            else:
                self.set_song_filter(before[0], exclude=before[1])

    def vt_redo_count(self) -> int:
        n = C.c_uint64()
        self.check(lib().shz_match_vt_redo(self.h, C.byref(n)))
        return n.value

    def spec_stats(self):
        """(queued, used): single small queries whose vote kernels were queued ahead of the vote count / that took
        their results from them."""
        a, b = C.c_uint64(), C.c_uint64()
        self.check(lib().shz_match_spec_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def mem_info(self):
        """(free, total) bytes of device memory right now."""
        a, b = C.c_uint64(), C.c_uint64()
        self.check(lib().shz_mem_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def alloc(self, nbytes) -> DevBuf:
        return DevBuf(self, nbytes)

    def host_array(self, shape, dtype=np.int16) -> np.ndarray:
        """numpy array in PINNED host memory (shz_host_alloc): PCM decoded into it reaches the GPU by DMA at the link rate.
        The memory lives as long as the array (and its views' base) does."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        p = vp()
        self.check(lib().shz_host_alloc(self.h, max(1, n * dt.itemsize), C.byref(p)))
        buf = (C.c_char * max(1, n * dt.itemsize)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
        addr = p.value
        import weakref
        weakref.finalize(buf, lambda: lib().shz_host_free(None, vp(addr)))   # (the array may outlive the context)
        return arr

    def sync(self):
        self.check(lib().shz_sync(self.h))

    def membw(self, mode: int = 0, nbytes: int = 4 << 30, iters: int = 5) -> float:
        """Measured HBM GB/s of a 16-B/lane stream: mode 0 copy (read + write), 1 read, 2 write."""
        g = C.c_float()
        self.check(lib().shz_membw(self.h, int(mode), int(nbytes), int(iters), C.byref(g)))
        return float(g.value)

    def sort_keys32(self, keys: np.ndarray, bit_lo: int = 0, bit_hi: int = 32, add: int = 0) -> np.ndarray:
        """Stable device radix sort of uint32 keys on bits [bit_lo, bit_hi); returns uint64 keys `key + add`."""
        k = np.ascontiguousarray(keys, np.uint32)
        out = np.empty(len(k), np.uint64)
        self.check(lib().shz_sort_keys32(self.h, ptr(k), len(k), int(bit_lo), int(bit_hi), int(add), ptr(out)))
        return out

    def sort_keys32_seg(self, keys: np.ndarray, seg_off, bit_lo: int = 0, bit_hi: int = 32) -> np.ndarray:
        """Segmented stable device radix sort of uint32 keys on bits [bit_lo, bit_hi): segment i = keys[seg_off[i] : seg_off[i + 1]]
        is ordered among itself (the vote passes: one segment per query)."""
        k = np.ascontiguousarray(keys, np.uint32)
        so = np.ascontiguousarray(seg_off, np.uint64)
        out = np.empty(len(k), np.uint32)
        self.check(lib().shz_sort_keys32_seg(self.h, ptr(k), so.ctypes.data_as(u64p), len(so) - 1, int(bit_lo), int(bit_hi), ptr(out)))
        return out

    def sort_pairs(self, keys: np.ndarray, vals=None, bit_lo: int = 0, bit_hi: int = 64):
        """Stable device radix sort of uint64 keys on bits [bit_lo, bit_hi), with an optional
        uint32 / uint64 payload; returns sorted copies."""
        k = np.ascontiguousarray(keys, np.uint64).copy()
        v, vb = None, 0
        if vals is not None:
            v = np.ascontiguousarray(vals).copy()
            vb = v.dtype.itemsize
            if vb not in (4, 8) or v.shape != k.shape:
                raise ValueError("payload must be 4 or 8 bytes per key")
        self.check(lib().shz_sort_pairs(self.h, k.ctypes.data, v.ctypes.data if v is not None else None, vb, k.size,
                                        int(bit_lo), int(bit_hi)))
        return (k, v) if v is not None else k

    def scan_prim(self, kind: int, values: np.ndarray, in_place: bool = False, want_total: bool = True):
        """The device exclusive scan of shz_prims.hip as the stages call it: kind SCAN_U32 (uint32 -> uint32), SCAN_POPC64
        (popcount of uint64 words -> uint32) or SCAN_U64 (uint64 -> uint64).  Returns (out, total); total is None without
        want_total (the device scan then gets no total pointer).  in_place: the device output is the device input."""
        x = np.ascontiguousarray(values, np.uint32 if kind == SCAN_U32 else np.uint64)
        out = np.empty(len(x), np.uint64 if kind == SCAN_U64 else np.uint32)
        tot = C.c_uint64(0xDEADBEEF)
        self.check(lib().shz_scan_host(self.h, int(kind), ptr(x), ptr(out), len(x), 1 if in_place else 0,
                                       C.byref(tot) if want_total else None))
        return out, (int(tot.value) if want_total else None)

    def set_workspace_limit(self, nbytes):
        self.check(lib().shz_set_workspace_limit(self.h, int(nbytes)))

    def release_workspace(self) -> int:
        n = C.c_uint64()
        self.check(lib().shz_release_workspace(self.h, C.byref(n)))
        return n.value

    def timer_start(self, slot=0):
        self.check(lib().shz_timer_start(self.h, slot))

    def timer_stop(self, slot=0) -> float:
        ms = C.c_float()
        self.check(lib().shz_timer_stop(self.h, slot, C.byref(ms)))
        return ms.value

    def set_profiling(self, on: bool):
        self.check(lib().shz_set_profiling(self.h, 1 if on else 0))

    def kernel_ms(self):
        names = ["stft_psd", "peak_pick", "peak_expand", "pair_hash", "peak_verify"]
        out = {}
        for i, n in enumerate(names):
            ms, k = C.c_float(), C.c_uint32()
            self.check(lib().shz_get_kernel_ms(self.h, i, C.byref(ms), C.byref(k)))
            out[n] = (ms.value, k.value)
        return out

    # ---- synthetic PCM ---------------------------------------------------------------------
    def synth_pcm(self, seed, clip0, n_clips, n_samples, tone_amp=0, noise_amp=8000, start=0, out: DevBuf = None) -> DevBuf:
        if out is None:
            out = self.alloc(int(n_clips) * int(n_samples) * 2)
        done = 0
        while done < n_clips:  # the kernel takes at most 65535 clips per launch
            k = min(65535, n_clips - done)
            self.check(lib().shz_synth_pcm(self.h, seed, clip0 + done, k, n_samples, tone_amp, noise_amp, start,
                                           vp(out.ptr + done * n_samples * 2)))
            done += k
        return out

    def synth_corpus(self, kind, seed, clip0, n_clips, n_samples, amp=3000, bed=100, burst=1500, start=0, out: DevBuf = None) -> DevBuf:
        """Music-like tracks (kind 1) or traffic-like noise (kind 2) on the device (twins: oracle/synth.music_clip / traffic_noise)."""
        if out is None:
            out = self.alloc(int(n_clips) * int(n_samples) * 2)
        done = 0
        while done < n_clips:
            k = min(65535, n_clips - done)
            self.check(lib().shz_synth_corpus(self.h, int(kind), seed, clip0 + done, k, n_samples, amp, bed, burst, start,
                                              vp(out.ptr + done * n_samples * 2)))
            done += k
        return out

    def mix_snr(self, sig: "DevBuf", noise: "DevBuf", n_clips: int, n_samples: int, snr_db: float, out: "DevBuf" = None) -> "DevBuf":
        """Per clip: noise scaled to the requested SNR (recognizer_test.py:426-435) and added; int16 out."""
        import math
        ss, sn = np.zeros(n_clips, np.uint64), np.zeros(n_clips, np.uint64)
        self.check(lib().shz_sumsq_i16(self.h, ptr(sig), n_clips, n_samples, ss.ctypes.data_as(u64p)))
        self.check(lib().shz_sumsq_i16(self.h, ptr(noise), n_clips, n_samples, sn.ctypes.data_as(u64p)))
        scale = np.empty(n_clips, np.float64)
        for c in range(n_clips):   # the reference's formula, evaluated exactly like oracle/synth.mix_query
            rms_s = math.sqrt(float(ss[c]) / n_samples)
            rms_n = math.sqrt(rms_s ** 2 / (pow(10, snr_db / 10)))
            rms_cur = math.sqrt(float(sn[c]) / n_samples)
            scale[c] = (rms_n / rms_cur) if rms_cur > 0 else 1.0
        if out is None:
            out = self.alloc(n_clips * n_samples * 2)
        self.check(lib().shz_mix_i16(self.h, ptr(sig), ptr(noise), n_clips, n_samples, scale.ctypes.data_as(f64p), ptr(out)))
        return out

    # ---- extraction ---------------------------------------------------------------------------
    @staticmethod
    def _clip_off(clip_off, n_clips=None):
        co = np.ascontiguousarray(clip_off, np.uint64)
        assert co.ndim == 1 and len(co) >= 1
        return co, len(co) - 1

    def upload_stats(self) -> dict:
        """Host PCM that went through the chunked upload pipeline since the context was created."""
        c, b, cs, ws = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double()
        self.check(lib().shz_upload_stats(self.h, C.byref(c), C.byref(b), C.byref(cs), C.byref(ws)))
        return {"chunks": c.value, "bytes": b.value, "copy_s": cs.value, "wait_s": ws.value}

    def set_overlap(self, noverlap: int):
        """noverlap of mlab.specgram for every later extraction call of this context (default 2048 = int(4096 * 0.5))."""
        self.check(lib().shz_set_overlap(self.h, int(noverlap)))
        self.hop = NFFT - int(noverlap)

    def frames_of(self, n_samples: int) -> int:
        return int(lib().shz_frame_count_hop(int(n_samples), int(getattr(self, "hop", HOP))))

    def set_stage_f64(self, enabled: bool):
        """fp64 staging of the power spectrogram (exact ties decided in the peak kernel) instead of fp32 + verify."""
        self.check(lib().shz_set_stage_f64(self.h, 1 if enabled else 0))

    def extract_stats(self) -> dict:
        v = [C.c_uint64() for _ in range(6)]
        self.check(lib().shz_extract_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("undecided", "decided_f64", "frames_recomputed", "f64_passes", "f64_clips", "f64_clip_frames"),
                        (int(x.value) for x in v)))

    def stft_db(self, pcm, clip_off, fs=44100, pcm_device=False, power=False):
        co, nc = self._clip_off(clip_off)
        frames = [self.frames_of(int(co[i + 1] - co[i])) for i in range(nc)]
        out = np.empty(sum(frames) * NBINS, np.float64)
        cnt = C.c_uint64()
        self.check(lib().shz_stft_db(self.h, ptr(pcm), co.ctypes.data_as(u64p), nc, fs,
                                     (PCM_DEVICE if pcm_device else 0) | (STFT_POWER if power else 0),
                                     ptr(out), out.size, C.byref(cnt)))
        res, pos = [], 0
        for f in frames:
            res.append(out[pos:pos + f * NBINS].reshape(NBINS, f))
            pos += f * NBINS
        return res

    def stft_stage(self, pcm, clip_off, fs=44100, kind=STAGE_F32, persistent=False) -> np.ndarray:
        """The rows stft_psd_kernel stages, [frames of all clips][2049], float32 (STAGE_F32: what fp32 peak picking reads) or
        float64 (STAGE_F64: the same arithmetic unrounded), launched as the extraction driver launches it; persistent: the
        persistent grid whatever the frame count.  For tests and tools."""
        x = np.ascontiguousarray(pcm, np.int16)
        co, nc = self._clip_off(clip_off)
        rows = sum(self.frames_of(int(co[i + 1] - co[i])) for i in range(nc))
        out = np.empty((rows, NBINS), np.float64 if kind == STAGE_F64 else np.float32)
        n = C.c_uint64()
        self.check(lib().shz_stft_stage_host(self.h, ptr(x), co.ctypes.data_as(u64p), nc, int(fs), int(kind),
                                             STAGE_PERSISTENT if persistent else 0, ptr(out), rows, C.byref(n)))
        assert n.value == rows, (n.value, rows)
        return out

    def set_numpy_product(self, fused: bool):
        """How the host's numpy forms conj(z) * z (see numpy_product_is_fused); set by __init__ from a probe."""
        self.check(lib().shz_set_numpy_product(self.h, 1 if fused else 0))

    def stft_db_any(self, x, fs=44100, nfft=2048, noverlap=1024, power=False) -> np.ndarray:
        """dB spectrogram [nfft/2 + 1, frames] of one channel for a window size other than 4096 (generic kernel)."""
        x = np.ascontiguousarray(x, np.int16)
        n = len(x)
        hop = int(nfft) - int(noverlap)
        frames = 1 if n < nfft or hop <= 0 else (n - int(nfft)) // hop + 1
        out = np.empty((int(nfft) // 2 + 1) * max(frames, 1), np.float64)
        nf = C.c_uint64()
        self.check(lib().shz_stft_db_any(self.h, ptr(x), n, int(fs), int(nfft), int(noverlap), STFT_POWER if power else 0, ptr(out),
                                         out.size, C.byref(nf)))
        return out[:(int(nfft) // 2 + 1) * nf.value].reshape(int(nfft) // 2 + 1, nf.value)

    def peaks(self, pcm, clip_off, fs=44100, amp_min=10.0, pcm_device=False):
        co, nc = self._clip_off(clip_off)
        total_frames = sum(self.frames_of(int(co[i + 1] - co[i])) for i in range(nc))
        cap = max(1024, total_frames * 16)
        flags = PCM_DEVICE if pcm_device else 0
        while True:
            pf, pt = np.empty(cap, np.uint16), np.empty(cap, np.uint32)
            po, cnt = np.zeros(nc + 1, np.uint64), C.c_uint64()
            rc = lib().shz_peaks(self.h, ptr(pcm), co.ctypes.data_as(u64p), nc, fs, float(amp_min), flags, ptr(pf), ptr(pt),
                                 po.ctypes.data_as(u64p), cap, C.byref(cnt))
            if rc == E_CAPACITY:
                cap = int(cnt.value)
                continue
            self.check(rc)
            n = int(cnt.value)
            return pf[:n], pt[:n], po

    def peaks_from_db(self, arr2d, amp_min=10.0):
        a = np.ascontiguousarray(arr2d, np.float64)
        assert a.ndim == 2
        cap = max(1024, a.shape[1] * 16)
        while True:
            of, ot, cnt = np.empty(cap, np.uint32), np.empty(cap, np.uint32), C.c_uint64()
            rc = lib().shz_peaks_from_db(self.h, ptr(a), a.shape[0], a.shape[1], float(amp_min), ptr(of), ptr(ot), cap, C.byref(cnt))
            if rc == E_CAPACITY:
                cap = int(cnt.value)
                continue
            self.check(rc)
            n = int(cnt.value)
            return of[:n], ot[:n]

    def pair_hash(self, peak_f, peak_t, peak_off, fan_value=5):
        pf = np.ascontiguousarray(peak_f, np.uint16)
        pt = np.ascontiguousarray(peak_t, np.uint32)
        po = np.ascontiguousarray(peak_off, np.uint64)
        nc = len(po) - 1
        cap = max(16, len(pf) * max(fan_value - 1, 0))
        k, t1 = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        ho, cnt = np.zeros(nc + 1, np.uint64), C.c_uint64()
        self.check(lib().shz_pair_hash(self.h, ptr(pf), ptr(pt), po.ctypes.data_as(u64p), nc, fan_value, ptr(k), ptr(t1),
                                       ho.ctypes.data_as(u64p), cap, C.byref(cnt)))
        n = int(cnt.value)
        return k[:n], t1[:n], ho

    def fingerprint_batch(self, pcm, clip_off, fs=44100, amp_min=10.0, fan_value=5, pcm_device=False,
                          out_key: DevBuf = None, out_t1: DevBuf = None, cap=None):
        """(key32, t1, hash_off).  With out_key/out_t1 DevBufs the hashes stay on the device and the
        returned arrays are None; hash_off (host) and the count are always returned."""
        co, nc = self._clip_off(clip_off)
        flags = PCM_DEVICE if pcm_device else 0
        ho, cnt = np.zeros(nc + 1, np.uint64), C.c_uint64()
        if out_key is not None:
            cap = int(cap if cap is not None else out_key.nbytes // 4)
            self.check(lib().shz_fingerprint_batch(self.h, ptr(pcm), co.ctypes.data_as(u64p), nc, fs, float(amp_min), fan_value,
                                                   flags | OUT_DEVICE, ptr(out_key), ptr(out_t1), ho.ctypes.data_as(u64p), cap,
                                                   C.byref(cnt)))
            return None, None, ho, int(cnt.value)
        total_frames = sum(self.frames_of(int(co[i + 1] - co[i])) for i in range(nc))
        cap = max(1024, total_frames * 40)
        while True:
            k, t1 = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
            rc = lib().shz_fingerprint_batch(self.h, ptr(pcm), co.ctypes.data_as(u64p), nc, fs, float(amp_min), fan_value, flags,
                                             ptr(k), ptr(t1), ho.ctypes.data_as(u64p), cap, C.byref(cnt))
            if rc == E_CAPACITY:
                cap = int(cnt.value)
                continue
            self.check(rc)
            n = int(cnt.value)
            return k[:n], t1[:n], ho, n

    def recognize_batch(self, table: "Table", pcm, clip_off, query_clip0, fs=44100, amp_min=10.0, fan_value=5, topn=2,
                        pcm_device=False, full_sort=False):
        """shz_recognize_batch: fingerprint the clips and match query q = clips [query_clip0[q], query_clip0[q + 1]) in one
        call, the hashes staying on the device.  Returns (res, ms_extract, ms_match), res as Table.match."""
        co, nc = self._clip_off(clip_off)
        qc = np.ascontiguousarray(query_clip0, np.uint32)
        nq = len(qc) - 1
        res = _match_result(nq, topn)
        me, mm = C.c_float(), C.c_float()
        self.check(lib().shz_recognize_batch(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, qc.ctypes.data_as(u32p), nq,
                                             int(fs), float(amp_min), int(fan_value), int(topn),
                                             (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0),
                                             ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]),
                                             ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"]), C.byref(me), C.byref(mm)))
        return res, float(me.value), float(mm.value)

    def _windows_with_room(self, call, room, cnt, cap_windows):
        """The two-call capacity idiom of the scans.  call(res, cap) -> rc runs the library call on the arrays res = room(n)
        with room for cap windows and leaves the total in cnt; without cap_windows the first call launches nothing and names
        the total.  Returns the arrays, cut to the total."""
        if cap_windows is None:
            rc = call(room(0), 0)
            if rc != E_CAPACITY:
                self.check(rc)
            cap_windows = int(cnt.value)
        res = room(int(cap_windows))
        self.check(call(res, cap_windows))
        n = int(cnt.value)
        return {k: v[:n] for k, v in res.items()}

    def scan_batch(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, fs=44100, amp_min=10.0,
                   fan_value=5, topn=2, pcm_device=False, full_sort=False, cap_windows=None):
        """shz_scan_batch: fingerprint the clips once and match every window of recording r = clips [rec_clip0[r],
        rec_clip0[r + 1]) in one call.  Returns (res, win_off, ms): res as Table.match over all windows, recording-major,
        win_off their CSR over the recordings, ms = (extract, window, match) device times.  cap_windows: the room handed
        to the library (default: what the frame counts give); too little raises E_CAPACITY, the total in the message."""
        co, nc = self._clip_off(clip_off)
        rc0 = np.ascontiguousarray(rec_clip0, np.uint32)
        nr = len(rc0) - 1
        flags = (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0)
        wo, cnt = np.zeros(nr + 1, np.uint64), C.c_uint64()
        ms = [C.c_float(), C.c_float(), C.c_float()]

        def call(res, cap):
            return lib().shz_scan_batch(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, rc0.ctypes.data_as(u32p), nr,
                                        int(fs), float(amp_min), int(fan_value), int(window_frames), int(step_frames), int(topn),
                                        flags, wo.ctypes.data_as(u64p), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]),
                                        ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"]), int(cap),
                                        C.byref(cnt), *[C.byref(m) for m in ms])
        res = self._windows_with_room(call, lambda n: _match_result(n, topn), cnt, cap_windows)
        return res, wo, tuple(float(m.value) for m in ms)

    # ---- the calls that return cells (shz_repeat.hip): repeats inside recordings, content shared between recordings, and that
    # at a table of warps.  Per family: what owns the cells (cell_off runs over it), and the arrays behind the cell arrays in
    # the order of the ABI -- name, dtype, what they run over
    _CELL_CALLS = {
        "repeats": ("rec", (("rec_hashes", np.uint32, "rec"), ("rec_skipped_keys", np.uint32, "rec"), ("rec_pairs", np.uint64, "rec"),
                            ("rec_skipped_rows", np.uint64, "rec"))),
        "shared": ("job", (("rec_hashes", np.uint32, "rec"), ("job_pairs", np.uint64, "job"), ("job_skipped_keys", np.uint32, "job"),
                           ("job_skipped_rows", np.uint64, "job"))),
        "shared_warps": ("job", (("rec_hashes", np.uint32, "rec"), ("job_hashes", np.uint32, "job"), ("job_pairs", np.uint64, "job"),
                                 ("job_skipped_keys", np.uint32, "job"), ("job_skipped_rows", np.uint64, "job"))),
    }

    def _cells_call(self, family, fn, nr, nj, cap_cells, fill, n_ms=0):
        """One call that returns cells and its capacity idiom.  fn(outs, tail) -> rc makes the library call: outs are the output
        arrays and the room as the ABI orders them, tail the count and the n_ms times behind them.  cap_cells None: a first call
        with no room names the count, a second one has it, checked; a number: that one call as it is.  fill: what the arrays
        hold beforehand (tests).  Returns (rc, out, count), and with n_ms (rc, out, count, ms): out = the CELL_FIELDS arrays (cut
        to the cells written; lag BIASED by SHARED_LAG_BIAS in the shared families, as the library returns it), cell_off over
        the family's owners, and the family's arrays per recording and per job; ms = the device times of the last call."""
        owner, arrays = self._CELL_CALLS[family]
        size = {"rec": nr, "job": nj}
        cnt = C.c_uint64(fill)
        ms = [C.c_float(float(np.float32(fill))) for _ in range(n_ms)]

        def call(cap):
            out = {k: np.full(int(cap), fill, np.uint32) for k in CELL_FIELDS}
            out["cell_off"] = np.full(size[owner] + 1, fill, np.uint64)
            out.update((name, np.full(size[over], fill, dtype)) for name, dtype, over in arrays)
            outs = [ptr(out["cell_off"]), *[ptr(out[k]) if cap else None for k in CELL_FIELDS], *[ptr(out[a[0]]) for a in arrays], int(cap)]
            return fn(outs, [C.byref(cnt), *[C.byref(m) for m in ms]]), out
        if cap_cells is None:
            rc, out = call(0)
            if rc == E_CAPACITY:
                rc, out = call(int(cnt.value))
            self.check(rc)
        else:
            rc, out = call(cap_cells)
        n = int(cnt.value)
        if rc in (OK, E_CAPACITY):
            for k in CELL_FIELDS:
                out[k] = out[k][:min(n, len(out[k]))]
        return (rc, out, n, tuple(float(m.value) for m in ms)) if n_ms else (rc, out, n)

    def _cells_with_room(self, raw, args, cap_cells):
        """A fused *_raw call with the room of the first call given: repeated once with the count it named, checked -> (out, ms)"""
        rc, out, n, ms = raw(*args, cap_cells)                         # (cap_cells None: both calls, checked)
        if rc == E_CAPACITY:
            rc, out, n, ms = raw(*args, n)
        self.check(rc)
        return out, ms

    @staticmethod
    def _host_columns(a, dtype_a, b, off, rec_clip0):
        """Two host columns, their CSR over the clips and the recordings' CSR as the ABI takes them; n_clips, n_recs"""
        off, rc0 = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(rec_clip0, np.uint32)
        return np.ascontiguousarray(a, dtype_a), np.ascontiguousarray(b, np.uint32), off, rc0, len(off) - 1, len(rc0) - 1

    def _pcm_clips(self, clip_off, rec_clip0):
        """clip_off and the recordings' CSR as the ABI takes them; n_clips, n_recs"""
        co, nc = self._clip_off(clip_off)
        rc0 = np.ascontiguousarray(rec_clip0, np.uint32)
        return co, rc0, nc, len(rc0) - 1

    # ---- repeated content inside recordings ------------------------------------------------------------------------------
    def repeats_hashes_raw(self, key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run=64, cell_shift=5, min_cell_pairs=8,
                           flags=0, cap_cells=None, fill=0):
        """One shz_repeats_hashes as it is on HOST columns: (rc, out, count) -- see _cells_call."""
        k, t, ho, rc0, nc, nr = self._host_columns(key32, np.uint32, t1, hash_off, rec_clip0)

        def fn(outs, tail):
            return lib().shz_repeats_hashes(self.h, ptr(k), ptr(t), ptr(ho), nc, ptr(rc0), nr, int(min_lag), int(max_lag),
                                            int(max_run), int(cell_shift), int(min_cell_pairs), int(flags), *outs, *tail)
        return self._cells_call("repeats", fn, nr, 0, cap_cells, fill)

    def repeats_hashes(self, key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run=64, cell_shift=5, min_cell_pairs=8):
        """shz_repeats_hashes (two calls): the repeat cells of recordings given as fingerprints -- host columns key32 / t1,
        hash_off their CSR over the clips, recording r = the clips [rec_clip0[r], rec_clip0[r + 1]).  Returns a dict: cell_off
        (CSR of the cells over the recordings), lag, block, pairs, first, last per cell, and rec_hashes, rec_pairs,
        rec_skipped_keys, rec_skipped_rows per recording."""
        _, out, _ = self.repeats_hashes_raw(key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run, cell_shift, min_cell_pairs)
        return out

    def repeats_batch_raw(self, pcm, clip_off, rec_clip0, min_lag, max_lag, max_run=64, cell_shift=5, min_cell_pairs=8, fs=44100,
                          amp_min=10.0, fan_value=5, pcm_device=False, cap_cells=None, fill=0):
        """One shz_repeats_batch as it is: (rc, out, count, ms) -- out as _cells_call, ms = (extract, pairs, cells) device
        times of the last call."""
        co, rc0, nc, nr = self._pcm_clips(clip_off, rec_clip0)

        def fn(outs, tail):
            return lib().shz_repeats_batch(self.h, ptr(pcm), ptr(co), nc, ptr(rc0), nr, int(fs), float(amp_min), int(fan_value),
                                           int(min_lag), int(max_lag), int(max_run), int(cell_shift), int(min_cell_pairs),
                                           PCM_DEVICE if pcm_device else 0, *outs, *tail)
        return self._cells_call("repeats", fn, nr, 0, cap_cells, fill, n_ms=3)

    def repeats_batch(self, pcm, clip_off, rec_clip0, min_lag, max_lag, max_run=64, cell_shift=5, min_cell_pairs=8, fs=44100,
                      amp_min=10.0, fan_value=5, pcm_device=False, cap_cells=None):
        """shz_repeats_batch: fingerprint the clips and find the repeat cells of recording r = clips [rec_clip0[r],
        rec_clip0[r + 1]) in one call, the hashes staying on the device.  cap_cells: the room of the first call (None: a call
        for the count, then one with that room -- the audio is fingerprinted twice; a number large enough: one call).  Returns
        (out, ms): out as repeats_hashes, ms = (extract, pairs, cells) device times."""
        args = (pcm, clip_off, rec_clip0, min_lag, max_lag, max_run, cell_shift, min_cell_pairs, fs, amp_min, fan_value, pcm_device)
        return self._cells_with_room(self.repeats_batch_raw, args, cap_cells)

    # ---- content shared between recordings (the job form of the join) ----------------------------------------------------
    @staticmethod
    def _jobs(jobs):
        """(a, b) pairs -> the two uint32 columns of the ABI"""
        j = np.asarray(list(jobs), np.uint32).reshape(-1, 2)
        return np.ascontiguousarray(j[:, 0]), np.ascontiguousarray(j[:, 1])

    def shared_hashes_raw(self, key32, t1, hash_off, rec_clip0, jobs, lag_lo, lag_hi, max_run=64, cell_shift=5, min_cell_pairs=8,
                          flags=0, cap_cells=None, fill=0):
        """One shz_shared_hashes as it is on HOST columns: (rc, out, count) -- see _cells_call.  jobs: (a, b) pairs."""
        k, t, ho, rc0, nc, nr = self._host_columns(key32, np.uint32, t1, hash_off, rec_clip0)
        ja, jb = self._jobs(jobs)

        def fn(outs, tail):
            return lib().shz_shared_hashes(self.h, ptr(k), ptr(t), ptr(ho), nc, ptr(rc0), nr, ptr(ja), ptr(jb), len(ja), int(lag_lo),
                                           int(lag_hi), int(max_run), int(cell_shift), int(min_cell_pairs), int(flags), *outs, *tail)
        return self._cells_call("shared", fn, nr, len(ja), cap_cells, fill)

    def shared_hashes(self, key32, t1, hash_off, rec_clip0, jobs, lag_lo, lag_hi, max_run=64, cell_shift=5, min_cell_pairs=8):
        """shz_shared_hashes (two calls): the cells of content shared between recordings given as fingerprints -- host columns
        key32 / t1, hash_off their CSR over the clips, recording r = the clips [rec_clip0[r], rec_clip0[r + 1]), jobs a list of
        (a, b): what of recording a also airs in recording b, at a lag t_b - t_a in [lag_lo, lag_hi] (signed frames).  Returns
        a dict: cell_off (CSR of the cells over the jobs), lag (BIASED: lag + SHARED_LAG_BIAS, the form repeats_fold takes),
        block, pairs, first, last per cell, rec_hashes per recording, job_pairs, job_skipped_keys, job_skipped_rows per job."""
        _, out, _ = self.shared_hashes_raw(key32, t1, hash_off, rec_clip0, jobs, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs)
        return out

    def shared_batch_raw(self, pcm, clip_off, rec_clip0, jobs, lag_lo, lag_hi, max_run=64, cell_shift=5, min_cell_pairs=8, fs=44100,
                         amp_min=10.0, fan_value=5, pcm_device=False, cap_cells=None, fill=0):
        """One shz_shared_batch as it is: (rc, out, count, ms) -- out as _cells_call, ms = (extract, pairs, cells) device times
        of the last call."""
        co, rc0, nc, nr = self._pcm_clips(clip_off, rec_clip0)
        ja, jb = self._jobs(jobs)

        def fn(outs, tail):
            return lib().shz_shared_batch(self.h, ptr(pcm), ptr(co), nc, ptr(rc0), nr, int(fs), float(amp_min), int(fan_value),
                                          ptr(ja), ptr(jb), len(ja), int(lag_lo), int(lag_hi), int(max_run), int(cell_shift),
                                          int(min_cell_pairs), PCM_DEVICE if pcm_device else 0, *outs, *tail)
        return self._cells_call("shared", fn, nr, len(ja), cap_cells, fill, n_ms=3)

    def shared_batch(self, pcm, clip_off, rec_clip0, jobs, lag_lo, lag_hi, max_run=64, cell_shift=5, min_cell_pairs=8, fs=44100,
                     amp_min=10.0, fan_value=5, pcm_device=False, cap_cells=None):
        """shz_shared_batch: fingerprint the clips -- every recording once, however many jobs name it -- and find the cells of
        every job (a, b) in one call, the hashes staying on the device.  cap_cells as repeats_batch.  Returns (out, ms): out as
        shared_hashes, ms = (extract, pairs, cells) device times."""
        args = (pcm, clip_off, rec_clip0, jobs, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs, fs, amp_min, fan_value, pcm_device)
        return self._cells_with_room(self.shared_batch_raw, args, cap_cells)

    # ---- altered content shared between recordings (the join at a table of warps) ----------------------------------------
    @staticmethod
    def _warp_jobs(jobs, tempos, pitches):
        """jobs (a, b, v, lag_lo, lag_hi) -> the five columns of the ABI; the warp table as two uint32 columns"""
        j = np.asarray(list(jobs), np.int64).reshape(-1, 5)
        cols = [np.ascontiguousarray(j[:, c], np.uint32) for c in range(3)] + [np.ascontiguousarray(j[:, c], np.int32) for c in (3, 4)]
        tq, fq = np.ascontiguousarray(tempos, np.uint32), np.ascontiguousarray(pitches, np.uint32)
        if tq.shape != fq.shape or tq.ndim != 1:
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        return cols, tq, fq

    def shared_warps_peaks_raw(self, peak_f, peak_t, peak_off, rec_clip0, tempos, pitches, jobs, max_run=64, cell_shift=5,
                               min_cell_pairs=8, fan_value=5, flags=0, cap_cells=None, fill=0):
        """One shz_shared_warps_peaks as it is on HOST peak lists: (rc, out, count) -- out as _cells_call, job_hashes among it.
        jobs: (a, b, v, lag_lo, lag_hi) tuples; warp v is (tempos[v], pitches[v]), Q16."""
        pf, pt, po, rc0, nc, nr = self._host_columns(peak_f, np.uint16, peak_t, peak_off, rec_clip0)
        cols, tq, fq = self._warp_jobs(jobs, tempos, pitches)
        nj = len(cols[0])

        def fn(outs, tail):
            return lib().shz_shared_warps_peaks(self.h, ptr(pf), ptr(pt), ptr(po), nc, ptr(rc0), nr, int(fan_value), ptr(tq), ptr(fq),
                                                len(tq), *[ptr(c) for c in cols], nj, int(max_run), int(cell_shift),
                                                int(min_cell_pairs), int(flags), *outs, *tail)
        return self._cells_call("shared_warps", fn, nr, nj, cap_cells, fill)

    def shared_warps_peaks(self, peak_f, peak_t, peak_off, rec_clip0, tempos, pitches, jobs, max_run=64, cell_shift=5,
                           min_cell_pairs=8, fan_value=5):
        """shz_shared_warps_peaks (two calls): the cells of altered content shared between recordings given as peak lists --
        host columns peak_f / peak_t in (t asc, f asc) order per clip, peak_off their CSR over the clips, recording r = the
        clips [rec_clip0[r], rec_clip0[r + 1]); jobs a list of (a, b, v, lag_lo, lag_hi): what of recording a, warped by
        (tempos[v], pitches[v]) (Q16), airs in b at a lag t_b - t'_a in the job's window.  Returns shared_hashes' dict (first,
        last, block in a's WARPED frames) plus job_hashes."""
        _, out, _ = self.shared_warps_peaks_raw(peak_f, peak_t, peak_off, rec_clip0, tempos, pitches, jobs, max_run, cell_shift,
                                                min_cell_pairs, fan_value)
        return out

    def shared_warps_batch_raw(self, pcm, clip_off, rec_clip0, tempos, pitches, jobs, max_run=64, cell_shift=5, min_cell_pairs=8,
                               fs=44100, amp_min=10.0, fan_value=5, pcm_device=False, cap_cells=None, fill=0):
        """One shz_shared_warps_batch as it is: (rc, out, count, ms) -- ms = (extract, warp, pairs, cells) device times of the
        last call."""
        co, rc0, nc, nr = self._pcm_clips(clip_off, rec_clip0)
        cols, tq, fq = self._warp_jobs(jobs, tempos, pitches)
        nj = len(cols[0])

        def fn(outs, tail):
            return lib().shz_shared_warps_batch(self.h, ptr(pcm), ptr(co), nc, ptr(rc0), nr, int(fs), float(amp_min), int(fan_value),
                                                ptr(tq), ptr(fq), len(tq), *[ptr(c) for c in cols], nj, int(max_run), int(cell_shift),
                                                int(min_cell_pairs), PCM_DEVICE if pcm_device else 0, *outs, *tail)
        return self._cells_call("shared_warps", fn, nr, nj, cap_cells, fill, n_ms=4)

    def shared_warps_batch(self, pcm, clip_off, rec_clip0, tempos, pitches, jobs, max_run=64, cell_shift=5, min_cell_pairs=8,
                           fs=44100, amp_min=10.0, fan_value=5, pcm_device=False, cap_cells=None):
        """shz_shared_warps_batch: the peaks of every clip once, one warp pass over every distinct (recording, warp) the jobs
        name, and the cells of every job in one call, the hashes staying on the device.  cap_cells as repeats_batch.  Returns
        (out, ms): out as shared_warps_peaks, ms = (extract, warp, pairs, cells) device times."""
        args = (pcm, clip_off, rec_clip0, tempos, pitches, jobs, max_run, cell_shift, min_cell_pairs, fs, amp_min, fan_value, pcm_device)
        return self._cells_with_room(self.shared_warps_batch_raw, args, cap_cells)

    def scan_extents_raw(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, min_aligned, max_gap=1,
                         margin_frames=0, d_tol=0, fs=44100, amp_min=10.0, fan_value=5, topn=2, pcm_device=False, full_sort=False,
                         cap_windows=0, cap_segs=0, hist=True, fill=0, zones=True, keep=None):
        """One shz_scan_extents as it is, with room for cap_windows windows and cap_segs segments: (rc, res, seg, zone,
        win_off, n_windows, n_segs, ms).  res as Table.match, seg as scan_timeline_raw's, zone = the arrays ZONE_FIELDS
        [cap_segs, 3] and hist [cap_segs, 3, 64] (None with hist false); seg and zone arrays are filled with `fill` before the
        call.  zones=False hands the library NULL zone arrays.  ms = (extract, window, match, extent).  keep ([cap_windows], bool):
        SHZ_SCAN_KEEP_MASK -- the windows with a false entry are cleared before the timeline."""
        co, nc = self._clip_off(clip_off)
        rc0 = np.ascontiguousarray(rec_clip0, np.uint32)
        nr = len(rc0) - 1
        flags = (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0)
        wo, cnt, scnt = np.zeros(nr + 1, np.uint64), C.c_uint64(), C.c_uint64()
        ms = [C.c_float(), C.c_float(), C.c_float(), C.c_float()]
        res = _match_result(int(cap_windows), topn)
        if keep is not None and int(cap_windows):
            if len(keep) != int(cap_windows):
                raise ValueError(f"keep has {len(keep)} entries for {int(cap_windows)} windows")
            res["nres"][:] = np.asarray(keep, bool)
            flags |= SCAN_KEEP_MASK
        seg = {k: np.full(int(cap_segs), fill, d) for k, d in SEGMENT_FIELDS}
        zone = {k: np.full((int(cap_segs), 3), fill, np.uint32) for k in ZONE_FIELDS}
        zone["hist"] = np.full((int(cap_segs), 3, 64), fill, np.uint32) if hist else None
        zp = [ptr(zone[k]) if zones else None for k in ZONE_FIELDS + ("hist",)]
        rc = lib().shz_scan_extents(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, rc0.ctypes.data_as(u32p), nr, int(fs),
                                    float(amp_min), int(fan_value), int(window_frames), int(step_frames), int(topn), flags,
                                    int(min_aligned), int(max_gap), int(margin_frames), int(d_tol), wo.ctypes.data_as(u64p),
                                    ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]), ptr(res["nres"]),
                                    ptr(res["nhash"]), ptr(res["npairs"]), int(cap_windows), C.byref(cnt),
                                    *[ptr(seg[k]) for k, _ in SEGMENT_FIELDS], int(cap_segs), C.byref(scnt), *zp,
                                    *[C.byref(m) for m in ms])
        return rc, res, seg, zone, wo, int(cnt.value), int(scnt.value), tuple(float(m.value) for m in ms)

    def scan_extents(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, min_aligned, max_gap=1,
                     margin_frames=0, d_tol=0, hist=True, keep=None, **kw):
        """shz_scan_extents: scan_batch, the timeline and the extent pass on every segment's three zones (whole, head, tail) in
        one call, the recordings' hashes staying on the device.  Returns (res, win_off, seg, zone, ms): res / win_off as
        scan_batch's, seg as scan_timeline's, zone = arrays lo, hi, count, q_first, q_last (recording frames), t_first, t_last
        (song frames), shift [n_segs, 3] and hist [n_segs, 3, 64] (None with hist false), ms = (extract, window, match, extent).
        Room: the window count follows from the frame counts (a first call that launches nothing), and there are never more
        segments than windows, so one call with room for that many suffices.  keep: see scan_extents_raw."""
        args = (table, pcm, clip_off, rec_clip0, window_frames, step_frames, min_aligned, max_gap, margin_frames, d_tol)
        rc, _, _, _, _, n_wins, _, _ = self.scan_extents_raw(*args, hist=False, **kw)
        if rc != E_CAPACITY:
            self.check(rc)
        rc, res, seg, zone, wo, n_wins, n_segs, ms = self.scan_extents_raw(*args, cap_windows=n_wins, cap_segs=n_wins, hist=hist,
                                                                           keep=keep, **kw)
        self.check(rc)
        return (res, wo, {k: v[:n_segs] for k, v in seg.items()},
                {k: (None if v is None else v[:n_segs]) for k, v in zone.items()}, ms)

    def scan_speeds(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, speeds, fs=44100, amp_min=10.0,
                    fan_value=5, topn=2, pcm_device=False, full_sort=False, cap_windows=None):
        """shz_scan_speeds: the peaks of the clips once, warped for every factor of `speeds` (Q16), every window of every
        recording matched at every rung on the device.  Returns (res, win_off, ms): res as scan_batch's (the best rung's
        rows) plus best [n_windows] (index into speeds) and profile [n_windows, K] (rank-0 aligned count of every rung);
        win_off the CSR of the windows over the recordings; ms = (extract, warp, window, match) device times."""
        co, nc = self._clip_off(clip_off)
        rc0 = np.ascontiguousarray(rec_clip0, np.uint32)
        sp = np.ascontiguousarray(speeds, np.uint32)
        nr = len(rc0) - 1
        flags = (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0)
        wo, cnt = np.zeros(nr + 1, np.uint64), C.c_uint64()
        ms = [C.c_float(), C.c_float(), C.c_float(), C.c_float()]

        def call(res, cap):
            return lib().shz_scan_speeds(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, rc0.ctypes.data_as(u32p), nr,
                                         int(fs), float(amp_min), int(fan_value), int(window_frames), int(step_frames), int(topn),
                                         sp.ctypes.data_as(u32p), len(sp), flags, wo.ctypes.data_as(u64p), ptr(res["best"]),
                                         ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]),
                                         ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"]), ptr(res["profile"]), int(cap),
                                         C.byref(cnt), *[C.byref(m) for m in ms])

        def room(n):
            res = _match_result(n, topn)
            res["best"], res["profile"] = np.zeros(n, np.uint32), np.zeros((n, len(sp)), np.uint32)
            return res
        res = self._windows_with_room(call, room, cnt, cap_windows)
        return res, wo, tuple(float(m.value) for m in ms)

    def scan_warps(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, tempos, pitches, select=None,
                   fs=44100, amp_min=10.0, fan_value=5, topn=2, pcm_device=False, full_sort=False, cap_windows=None):
        """shz_scan_warps: scan_speeds with a time and a frequency factor of its own for every variant (warp v is (tempos[v],
        pitches[v]), Q16).  select=(sel_off, sel_warp): window w tries the warps sel_warp[sel_off[w]:sel_off[w + 1]] only
        (strictly ascending; the windows recording-major), and profile is slot-aligned ([sel_off[-1]]) instead of
        [n_windows, n_warps]; a window with an empty list has best = SCAN_NO_WARP; a sel_off that has not one entry more
        than there are windows is a ValueError.  Returns (res, win_off, ms) as scan_speeds, res with "work" = (warped hash
        entries written, window entries handed to the match)."""
        co, nc = self._clip_off(clip_off)
        rc0 = np.ascontiguousarray(rec_clip0, np.uint32)
        tq, fq = np.ascontiguousarray(tempos, np.uint32), np.ascontiguousarray(pitches, np.uint32)
        if tq.shape != fq.shape or tq.ndim != 1:
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        so = sw = None
        if select is not None:
            so, sw = np.ascontiguousarray(select[0], np.uint64), np.ascontiguousarray(select[1], np.uint32)
            if len(so) < 1 or len(sw) < int(so.max(initial=0)):
                raise ValueError("select=(sel_off, sel_warp): sel_off is a CSR over the windows into sel_warp")
        nr = len(rc0) - 1
        flags = (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0)
        wo, cnt, work = np.zeros(nr + 1, np.uint64), C.c_uint64(), np.zeros(2, np.uint64)
        ms = [C.c_float(), C.c_float(), C.c_float(), C.c_float()]
        prof = {}

        def call(res, cap):
            # without cap_windows the first call has counted the windows and launched nothing: a sel_off of another length
            # is refused here, before the library reads it
            if select is not None and cap and len(so) != int(cap) + 1:
                raise ValueError(f"select: sel_off has {len(so)} entries for {int(cap)} windows")
            return lib().shz_scan_warps(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, rc0.ctypes.data_as(u32p), nr,
                                        int(fs), float(amp_min), int(fan_value), int(window_frames), int(step_frames), int(topn),
                                        tq.ctypes.data_as(u32p), fq.ctypes.data_as(u32p), len(tq),
                                        None if so is None else so.ctypes.data_as(u64p),
                                        None if sw is None else sw.ctypes.data_as(u32p), flags, wo.ctypes.data_as(u64p),
                                        ptr(res["best"]), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]),
                                        ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"]), ptr(prof["profile"]),
                                        work.ctypes.data_as(u64p), int(cap), C.byref(cnt), *[C.byref(m) for m in ms])

        def room(n):
            res = _match_result(n, topn)
            res["best"] = np.zeros(n, np.uint32)
            prof["profile"] = np.zeros((n, len(tq)), np.uint32) if select is None else np.zeros(int(so[-1]) if n else 0, np.uint32)
            return res
        res = self._windows_with_room(call, room, cnt, cap_windows)
        if select is not None and len(so) != int(cnt.value) + 1:      # (a cap_windows of the caller's above the total)
            raise ValueError(f"select: sel_off has {len(so)} entries for {int(cnt.value)} windows")
        res["profile"] = prof["profile"][:int(cnt.value)] if select is None else prof["profile"]
        res["work"] = (int(work[0]), int(work[1]))
        return res, wo, tuple(float(m.value) for m in ms)

    def scan_plays_raw(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, seg, margin_frames=0,
                       drift_bins=0, fs=44100, amp_min=10.0, fan_value=5, pcm_device=False, hist=True, fill=0, work=True):
        """One shz_scan_plays as it is: (rc, zone, work, ms).  seg = the arrays PLAY_SEGMENT_FIELDS of the caller's segments
        (a warped timeline's, each with its own Q16 pair t16 / f16).  zone = the arrays PLAY_ZONE_FIELDS [n_segs, 3] and hist
        [n_segs, 3, 64] (None with hist false), filled with `fill` before the call; work = (peak items warped, hash entries
        written, zone entries handed to the extent pass); ms = (extract, warp, extent)."""
        co, nc = self._clip_off(clip_off)
        rc0 = np.ascontiguousarray(rec_clip0, np.uint32)
        a = _play_segments(seg)
        n = len(a["rec"])
        zone = {k: np.full((n, 3), fill, d) for k, d in PLAY_ZONE_FIELDS}
        zone["hist"] = np.full((n, 3, 64), fill, np.uint32) if hist else None
        wk = np.full(3, fill, np.uint64)
        ms = [C.c_float(), C.c_float(), C.c_float()]
        rc = lib().shz_scan_plays(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, rc0.ctypes.data_as(u32p), len(rc0) - 1,
                                  int(fs), float(amp_min), int(fan_value), int(window_frames), int(step_frames),
                                  PCM_DEVICE if pcm_device else 0, *[ptr(a[k]) for k, _ in PLAY_SEGMENT_FIELDS], n,
                                  int(margin_frames), int(drift_bins), *[ptr(zone[k]) for k, _ in PLAY_ZONE_FIELDS[:10]],
                                  ptr(zone["hist"]), *[ptr(zone[k]) for k, _ in PLAY_ZONE_FIELDS[10:]],
                                  ptr(wk) if work else None, *[C.byref(m) for m in ms])
        return rc, zone, tuple(int(x) for x in wk), tuple(float(m.value) for m in ms)

    def scan_plays(self, table: "Table", pcm, clip_off, rec_clip0, window_frames, step_frames, seg, margin_frames=0, drift_bins=0,
                   **kw):
        """shz_scan_plays: the extent pass with the moments on the three zones (whole, head, tail) of every
        segment of a warped scan, each cut from hash lists warped at the segment's own pair, which never leave the device.
        Returns (zone, work, ms): zone = arrays lo, hi (own recording frames), d_lo, d_hi (the candidate), count, q_first,
        q_last (WARPED recording frames), t_first, t_last (song frames), shift, sum_q, sum_u, sum_qq, sum_qu [n_segs, 3] and
        hist [n_segs, 3, 64]; work and ms as scan_plays_raw."""
        rc, zone, work, ms = self.scan_plays_raw(table, pcm, clip_off, rec_clip0, window_frames, step_frames, seg, margin_frames,
                                                 drift_bins, **kw)
        self.check(rc)
        return zone, work, ms

    def warp_pair_hash_raw(self, peak_f, peak_t, peak_off, speeds, query_clip0=None, fan_value=5, cap=0, device_in=False,
                           out_key: DevBuf = None, out_t1: DevBuf = None):
        """One shz_warp_pair_hash as it is: (rc, key32, t1, hash_off, count) without retrying.  peak_f / peak_t: host
        arrays, or DevBufs with device_in.  With out_key / out_t1 DevBufs the hashes stay on the device and the returned
        arrays are None."""
        po = np.ascontiguousarray(peak_off, np.uint64)
        sp = np.ascontiguousarray(speeds, np.uint32)
        nc = len(po) - 1
        qc = None if query_clip0 is None else np.ascontiguousarray(query_clip0, np.uint32)
        if not device_in:
            peak_f, peak_t = np.ascontiguousarray(peak_f, np.uint16), np.ascontiguousarray(peak_t, np.uint32)
        ho, cnt = np.zeros(nc * len(sp) + 1, np.uint64), C.c_uint64()
        flags = (IN_DEVICE if device_in else 0) | (OUT_DEVICE if out_key is not None else 0)
        k = t1 = None
        if out_key is None:
            k, t1 = np.empty(max(int(cap), 1), np.uint32), np.empty(max(int(cap), 1), np.uint32)
        rc = lib().shz_warp_pair_hash(self.h, ptr(peak_f), ptr(peak_t), po.ctypes.data_as(u64p), nc,
                                      None if qc is None else qc.ctypes.data_as(u32p), 0 if qc is None else len(qc) - 1,
                                      sp.ctypes.data_as(u32p), len(sp), int(fan_value), flags,
                                      ptr(out_key if out_key is not None else k), ptr(out_t1 if out_key is not None else t1),
                                      ho.ctypes.data_as(u64p), int(cap), C.byref(cnt))
        n = int(cnt.value)
        if k is not None:
            k, t1 = k[:min(n, int(cap))], t1[:min(n, int(cap))]
        return rc, k, t1, ho, n

    def warp_pair_hash(self, peak_f, peak_t, peak_off, speeds, query_clip0=None, fan_value=5):
        """shz_warp_pair_hash (two calls: count, then write): (key32, t1, hash_off) in the order query, speed, clip."""
        rc, k, t1, ho, n = self.warp_pair_hash_raw(peak_f, peak_t, peak_off, speeds, query_clip0, fan_value, 0)
        if rc == E_CAPACITY:
            rc, k, t1, ho, n = self.warp_pair_hash_raw(peak_f, peak_t, peak_off, speeds, query_clip0, fan_value, n)
        self.check(rc)
        return k[:n], t1[:n], ho

    def recognize_speeds(self, table: "Table", pcm, clip_off, query_clip0, speeds, fs=44100, amp_min=10.0, fan_value=5, topn=2,
                         pcm_device=False, full_sort=False, extents=False, drift_bins=0):
        """shz_recognize_speeds: the peaks of the clips once, every factor of `speeds` (Q16) warped, hashed and matched on
        the device.  Returns (res, ms): res as Table.match over the queries (the best variant's rows; no npairs) plus
        best [nq] (index into speeds) and profile [nq, K] (rank-0 aligned count of every variant); ms = (extract, warp,
        match) device times.  extents / drift_bins: as recognize_warps' (shz_recognize_speeds_extents)."""
        if extents:
            sp = np.ascontiguousarray(speeds, np.uint32)
            return self._recognize_extents("shz_recognize_speeds_extents", table, pcm, clip_off, query_clip0, [sp], fs, amp_min,
                                           fan_value, topn, pcm_device, full_sort, drift_bins)
        co, nc = self._clip_off(clip_off)
        qc = np.ascontiguousarray(query_clip0, np.uint32)
        sp = np.ascontiguousarray(speeds, np.uint32)
        nq = len(qc) - 1
        res = _match_result(nq, topn)
        del res["npairs"]
        res["best"], res["profile"] = np.zeros(nq, np.uint32), np.zeros((nq, len(sp)), np.uint32)
        ms = [C.c_float(), C.c_float(), C.c_float()]
        self.check(lib().shz_recognize_speeds(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, qc.ctypes.data_as(u32p), nq,
                                              int(fs), float(amp_min), int(fan_value), int(topn), sp.ctypes.data_as(u32p), len(sp),
                                              (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0),
                                              ptr(res["best"]), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]),
                                              ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]), ptr(res["profile"]),
                                              *[C.byref(m) for m in ms]))
        return res, tuple(float(m.value) for m in ms)

    def warp_pair_hash_tf_raw(self, peak_f, peak_t, peak_off, tempos, pitches, query_clip0=None, fan_value=5, cap=0,
                              device_in=False, out_key: DevBuf = None, out_t1: DevBuf = None):
        """One shz_warp_pair_hash_tf as it is: (rc, key32, t1, hash_off, count) without retrying; warp v is (tempos[v],
        pitches[v]), Q16.  Buffers as for warp_pair_hash_raw."""
        po = np.ascontiguousarray(peak_off, np.uint64)
        tq, fq = np.ascontiguousarray(tempos, np.uint32), np.ascontiguousarray(pitches, np.uint32)
        if tq.shape != fq.shape or tq.ndim != 1:
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        nc = len(po) - 1
        qc = None if query_clip0 is None else np.ascontiguousarray(query_clip0, np.uint32)
        if not device_in:
            peak_f, peak_t = np.ascontiguousarray(peak_f, np.uint16), np.ascontiguousarray(peak_t, np.uint32)
        ho, cnt = np.zeros(nc * len(tq) + 1, np.uint64), C.c_uint64()
        flags = (IN_DEVICE if device_in else 0) | (OUT_DEVICE if out_key is not None else 0)
        k = t1 = None
        if out_key is None:
            k, t1 = np.empty(max(int(cap), 1), np.uint32), np.empty(max(int(cap), 1), np.uint32)
        rc = lib().shz_warp_pair_hash_tf(self.h, ptr(peak_f), ptr(peak_t), po.ctypes.data_as(u64p), nc,
                                         None if qc is None else qc.ctypes.data_as(u32p), 0 if qc is None else len(qc) - 1,
                                         tq.ctypes.data_as(u32p), fq.ctypes.data_as(u32p), len(tq), int(fan_value), flags,
                                         ptr(out_key if out_key is not None else k), ptr(out_t1 if out_key is not None else t1),
                                         ho.ctypes.data_as(u64p), int(cap), C.byref(cnt))
        n = int(cnt.value)
        if k is not None:
            k, t1 = k[:min(n, int(cap))], t1[:min(n, int(cap))]
        return rc, k, t1, ho, n

    def warp_pair_hash_tf(self, peak_f, peak_t, peak_off, tempos, pitches, query_clip0=None, fan_value=5):
        """shz_warp_pair_hash_tf (two calls: count, then write): (key32, t1, hash_off) in the order query, warp, clip."""
        rc, k, t1, ho, n = self.warp_pair_hash_tf_raw(peak_f, peak_t, peak_off, tempos, pitches, query_clip0, fan_value, 0)
        if rc == E_CAPACITY:
            rc, k, t1, ho, n = self.warp_pair_hash_tf_raw(peak_f, peak_t, peak_off, tempos, pitches, query_clip0, fan_value, n)
        self.check(rc)
        return k[:n], t1[:n], ho

    def _recognize_extents(self, symbol, table, pcm, clip_off, query_clip0, ladders, fs, amp_min, fan_value, topn, pcm_device,
                           full_sort, drift_bins):
        """shz_recognize_warps_extents (ladders = [tempos, pitches]) / shz_recognize_speeds_extents (ladders = [speeds]): (res,
        ms) with the extent arrays in res and ms = (extract, warp, match, extent)"""
        co, nc = self._clip_off(clip_off)
        qc = np.ascontiguousarray(query_clip0, np.uint32)
        nq, K = len(qc) - 1, len(ladders[0])
        res = _match_result(nq, topn)
        del res["npairs"]
        res["best"], res["profile"] = np.zeros(nq, np.uint32), np.zeros((nq, K), np.uint32)
        ext32, ext64 = ("count", "q_first", "q_last", "t_first", "t_last"), ("sum_q", "sum_u", "sum_qq", "sum_qu")
        res.update({k: np.zeros((nq, topn), np.uint32) for k in ext32})
        res.update({k: np.zeros((nq, topn), np.uint64) for k in ext64})
        res["hist"], res["shift"] = np.zeros((nq, topn, 64), np.uint32), np.zeros(nq, np.uint32)
        ms = [C.c_float(), C.c_float(), C.c_float(), C.c_float()]
        self.check(getattr(lib(), symbol)(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, qc.ctypes.data_as(u32p), nq,
                                          int(fs), float(amp_min), int(fan_value), int(topn),
                                          *[a.ctypes.data_as(u32p) for a in ladders], K,
                                          (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0),
                                          ptr(res["best"]), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]),
                                          ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]), ptr(res["profile"]),
                                          *[C.byref(m) for m in ms[:3]], int(drift_bins), *[ptr(res[k]) for k in ext32 + ext64],
                                          ptr(res["hist"]), ptr(res["shift"]), C.byref(ms[3])))
        return res, tuple(float(m.value) for m in ms)

    def recognize_warps(self, table: "Table", pcm, clip_off, query_clip0, tempos, pitches, fs=44100, amp_min=10.0, fan_value=5,
                        topn=2, pcm_device=False, full_sort=False, extents=False, drift_bins=0):
        """shz_recognize_warps: recognize_speeds with a time and a frequency factor of its own for every variant (warp v is
        (tempos[v], pitches[v]), Q16).  Returns (res, ms) shaped as recognize_speeds': best [nq] indexes the warps, profile
        is [nq, n_warps].
        extents (shz_recognize_warps_extents): the extent pass on the best variant's hashes, candidate n of query q being
        (sid[q, n], delta[q, n] - w, delta[q, n] + w) with w = the vote tolerance + drift_bins.  res gains count, q_first,
        q_last, t_first, t_last [nq, topn] (q_* in WARPED frames, as delta), the moments sum_q, sum_u, sum_qq, sum_qu
        [nq, topn] (uint64; extent.line_fit), hist [nq, topn, 64] and shift [nq]; ms gains a fourth entry, the extent
        stage."""
        co, nc = self._clip_off(clip_off)
        qc = np.ascontiguousarray(query_clip0, np.uint32)
        tq, fq = np.ascontiguousarray(tempos, np.uint32), np.ascontiguousarray(pitches, np.uint32)
        if tq.shape != fq.shape or tq.ndim != 1:
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        if extents:
            return self._recognize_extents("shz_recognize_warps_extents", table, pcm, clip_off, query_clip0, [tq, fq], fs, amp_min,
                                           fan_value, topn, pcm_device, full_sort, drift_bins)
        nq = len(qc) - 1
        res = _match_result(nq, topn)
        del res["npairs"]
        res["best"], res["profile"] = np.zeros(nq, np.uint32), np.zeros((nq, len(tq)), np.uint32)
        ms = [C.c_float(), C.c_float(), C.c_float()]
        self.check(lib().shz_recognize_warps(self.h, table.h, ptr(pcm), co.ctypes.data_as(u64p), nc, qc.ctypes.data_as(u32p), nq,
                                             int(fs), float(amp_min), int(fan_value), int(topn), tq.ctypes.data_as(u32p),
                                             fq.ctypes.data_as(u32p), len(tq),
                                             (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0),
                                             ptr(res["best"]), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]),
                                             ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]), ptr(res["profile"]),
                                             *[C.byref(m) for m in ms]))
        return res, tuple(float(m.value) for m in ms)

    def warp_rows_raw(self, key32, off, row_off, tempos, pitches, cap=0, device_in=False, out_key: DevBuf = None,
                      out_off: DevBuf = None):
        """One shz_warp_rows as it is: (rc, key32, off, out_row_off, count) without retrying; warp v is (tempos[v],
        pitches[v]), Q16.  key32 / off: host arrays, or DevBufs with device_in.  With out_key / out_off DevBufs the warped
        rows stay on the device and the returned arrays are None."""
        ro = np.ascontiguousarray(row_off, np.uint64)
        tq, fq = np.ascontiguousarray(tempos, np.uint32), np.ascontiguousarray(pitches, np.uint32)
        if tq.shape != fq.shape or tq.ndim != 1:
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        ns = len(ro) - 1
        if not device_in:
            key32, off = np.ascontiguousarray(key32, np.uint32), np.ascontiguousarray(off, np.uint32)
        oro, cnt = np.zeros(ns * len(tq) + 1, np.uint64), C.c_uint64()
        flags = (IN_DEVICE if device_in else 0) | (OUT_DEVICE if out_key is not None else 0)
        k = o = None
        if out_key is None:
            k, o = np.empty(max(int(cap), 1), np.uint32), np.empty(max(int(cap), 1), np.uint32)
        rc = lib().shz_warp_rows(self.h, ptr(key32), ptr(off), ro.ctypes.data_as(u64p), ns, tq.ctypes.data_as(u32p),
                                 fq.ctypes.data_as(u32p), len(tq), flags, ptr(out_key if out_key is not None else k),
                                 ptr(out_off if out_key is not None else o), oro.ctypes.data_as(u64p), int(cap), C.byref(cnt))
        n = int(cnt.value)
        if k is not None:
            k, o = k[:min(n, int(cap))], o[:min(n, int(cap))]
        return rc, k, o, oro, n

    def warp_rows(self, key32, off, row_off, tempos, pitches):
        """shz_warp_rows (two calls: count, then write): the rows of every song at every warp, (key32, off, out_row_off) in
        the order song, warp; out_row_off has n_songs * n_warps + 1 entries."""
        rc, k, o, oro, n = self.warp_rows_raw(key32, off, row_off, tempos, pitches, 0)
        if rc == E_CAPACITY:
            rc, k, o, oro, n = self.warp_rows_raw(key32, off, row_off, tempos, pitches, n)
        self.check(rc)
        return k[:n], o[:n], oro

    def resample_raw(self, pcm, clip_off, L, M, T, taps, in_base=None, m_first=None, m_end=None, pcm_device=False,
                     out: DevBuf = None, cap=None):
        """One shz_resample_i16 as it is: (rc, out, out_off, count) without retrying.  taps: int32 [L, T] in Q30.  With `out`
        a DevBuf the samples stay on the device (cap in samples, default its size) and the returned array is None; else
        a host array of cap samples is filled."""
        co, nc = self._clip_off(clip_off)
        tp = np.ascontiguousarray(taps, np.int32)
        opt = [None if a is None else np.ascontiguousarray(a, np.uint64) for a in (in_base, m_first, m_end)]
        oo, cnt = np.zeros(nc + 1, np.uint64), C.c_uint64()
        flags = PCM_DEVICE if pcm_device else 0
        if out is not None:
            cap = int(out.nbytes // 2 if cap is None else cap)
            host = None
        else:
            if cap is None:   # room for every output asked for
                cap = (int(np.sum(opt[2] - opt[1])) if opt[1] is not None and opt[2] is not None else
                       sum(-(-int(co[i + 1] - co[i]) * int(L) // max(int(M), 1)) for i in range(nc)))
            host = np.empty(max(int(cap), 1), np.int16)
        rc = lib().shz_resample_i16(self.h, ptr(pcm), co.ctypes.data_as(u64p), nc, int(L), int(M), int(T), ptr(tp), ptr(opt[0]),
                                    ptr(opt[1]), ptr(opt[2]), flags | (OUT_DEVICE if out is not None else 0),
                                    ptr(out if out is not None else host), oo.ctypes.data_as(u64p), int(cap), C.byref(cnt))
        n = int(cnt.value)
        return rc, (None if host is None else host[:min(n, int(cap))]), oo, n

    def resample(self, pcm, clip_off, L, M, T, taps, in_base=None, m_first=None, m_end=None, pcm_device=False, device_out=False):
        """Polyphase resampling of a batch (shz_resample_i16): (samples, out_off), clip c's at [out_off[c], out_off[c + 1]).
        device_out: samples is a DevBuf the caller frees, and the PCM never visits the host."""
        co, nc = self._clip_off(clip_off)
        if m_first is not None:
            total = int(np.sum(np.asarray(m_end, np.uint64) - np.asarray(m_first, np.uint64)))
        else:
            total = sum(-(-int(co[i + 1] - co[i]) * int(L) // int(M)) for i in range(nc))
        buf = self.alloc(max(total, 1) * 2) if device_out else None
        rc, out, oo, _ = self.resample_raw(pcm, co, L, M, T, taps, in_base, m_first, m_end, pcm_device, buf, total)
        if rc != OK and buf is not None:
            buf.free()
        self.check(rc)
        return (buf if device_out else out), oo

    def resample_kernel_ms(self):
        """(ms, launches) of the resample kernel since set_profiling(True) (shz_get_kernel_ms slot 5)."""
        ms, k = C.c_float(), C.c_uint32()
        self.check(lib().shz_get_kernel_ms(self.h, 5, C.byref(ms), C.byref(k)))
        return ms.value, k.value

    def sha1_prefix(self, key32, device=False, n=None) -> np.ndarray:
        if not device:
            key32 = np.ascontiguousarray(key32, np.uint32)
            n = len(key32)
        out = np.empty((int(n), 10), np.uint8)
        self.check(lib().shz_sha1_prefix(self.h, ptr(key32), int(n), IN_DEVICE if device else 0, ptr(out)))
        return out


def _sha1_invert(self, digests10: np.ndarray) -> np.ndarray:
    """key32 of each 10-byte digest (0xFFFFFFFF where none): brute force over the preimage space on the GPU."""
    d = np.ascontiguousarray(digests10, np.uint8).reshape(-1, 10)
    out = np.empty(len(d), np.uint32)
    self.check(lib().shz_sha1_invert(self.h, ptr(d), len(d), ptr(out)))
    return out


Context.sha1_invert = _sha1_invert


def _match_result(nq: int, topn: int) -> dict:
    """Zeroed output arrays of a match over nq queries (include/shz.h at shz_match_batch)."""
    return {
        "sid": np.zeros((nq, topn), np.uint32), "delta": np.zeros((nq, topn), np.int32),
        "aligned": np.zeros((nq, topn), np.uint32), "dedup": np.zeros((nq, topn), np.uint32),
        "nres": np.zeros(nq, np.uint32), "nhash": np.zeros(nq, np.uint32), "npairs": np.zeros(nq, np.uint64)}


def warp_row_host(key32, off, t16: int, f16: int):
    """shz_warp_row_host (host only): the row warp's map over host arrays -- (key32', off', keep), elementwise; where
    keep is False the two outputs are 0."""
    k, o = np.ascontiguousarray(key32, np.uint32).reshape(-1), np.ascontiguousarray(off, np.uint32).reshape(-1)
    if k.shape != o.shape:
        raise ValueError("key32 and off are two columns of one length")
    ok, oo, keep = np.zeros(len(k), np.uint32), np.zeros(len(k), np.uint32), np.zeros(len(k), np.uint8)
    rc = lib().shz_warp_row_host(ptr(k), ptr(o), len(k), int(t16), int(f16), ptr(ok), ptr(oo), ptr(keep))
    if rc != OK:
        raise ShzError(rc, "shz_warp_row_host: factors are Q16 in [32768, 131072]")
    return ok, oo, keep.astype(bool)


def recognize_estimate(frames: int, fan_value: int = 5) -> int:
    """shz_recognize_estimate (host only): entries the first extraction pass of the fused call has room for."""
    return int(lib().shz_recognize_estimate(int(frames), int(fan_value)))


def scan_window_count(frames: int, window_frames: int, step_frames: int) -> int:
    """shz_scan_window_count (host only): windows of a recording of `frames` frames (0 frames: no clips, no window)."""
    return int(lib().shz_scan_window_count(int(frames), int(window_frames), int(step_frames)))


SEGMENT_FIELDS = (("rec", np.uint32), ("sid", np.uint32), ("shift", np.int64), ("first", np.uint32), ("last", np.uint32),
                  ("hits", np.uint32), ("best", np.uint32))


def _timeline_raw(fn, fields, win_off, sid, delta, aligned, nres, step_frames, min_aligned, max_gap, cap, best=None, tables=(),
                  tols=()):
    """One call of a timeline fold as it is (host only): (rc, segments, count) with room for `cap` segments.  best, tables and
    tols are what the variants' folds take beside the plain one's arguments."""
    wo = np.ascontiguousarray(win_off, np.uint64)
    sid, delta, aligned = (np.ascontiguousarray(a, d) for a, d in ((sid, np.uint32), (delta, np.int32), (aligned, np.uint32)))
    nres = np.ascontiguousarray(nres, np.uint32)
    tabs = [np.ascontiguousarray(t, np.uint32) for t in tables]
    nw = len(nres)
    topn = 1 if sid.ndim == 1 else int(sid.shape[1])
    assert sid.shape == delta.shape == aligned.shape and sid.size == nw * topn and int(wo[-1]) - int(wo[0]) <= nw
    assert all(len(t) == len(tabs[0]) for t in tabs)
    variant, ladder = [], []
    if best is not None:
        best = np.ascontiguousarray(best, np.uint32)
        assert len(best) == nw
        variant, ladder = [ptr(best)], [t.ctypes.data_as(u32p) for t in tabs] + [len(tabs[0])]
    seg = {k: np.zeros(int(cap), d) for k, d in fields}
    cnt = C.c_uint64()
    rc = fn(wo.ctypes.data_as(u64p), len(wo) - 1, ptr(sid), ptr(delta), ptr(aligned), ptr(nres), *variant, topn, int(step_frames),
            *ladder, int(min_aligned), int(max_gap), *[int(x) for x in tols], *[ptr(seg[k]) if cap else None for k, _ in fields],
            int(cap), C.byref(cnt))
    return rc, seg, int(cnt.value)


def _timeline(raw, name, *args) -> dict:
    """The two calls of a timeline fold: one for the count, one with that much room."""
    rc, seg, n = raw(*args, 0)
    if rc == E_CAPACITY:
        rc, seg, n = raw(*args, n)
    if rc != OK:
        raise ShzError(rc, name + ": bad arguments")
    return seg


def scan_timeline_raw(win_off, sid, delta, aligned, nres, step_frames, min_aligned, max_gap=1, cap=0):
    """One shz_scan_timeline as it is (host only): (rc, segments, count) with room for `cap` segments."""
    return _timeline_raw(lib().shz_scan_timeline, SEGMENT_FIELDS, win_off, sid, delta, aligned, nres, step_frames, min_aligned,
                         max_gap, cap)


def scan_timeline(win_off, sid, delta, aligned, nres, step_frames, min_aligned, max_gap=1) -> dict:
    """shz_scan_timeline (host only, two calls): the rank-0 answers of a scan folded into segments -- arrays rec, sid, shift
    (song frame - recording frame), first / last (windows of the recording), hits, best (largest aligned count)."""
    return _timeline(scan_timeline_raw, "shz_scan_timeline", win_off, sid, delta, aligned, nres, step_frames, min_aligned, max_gap)


CELL_FIELDS = ("lag", "block", "pairs", "first", "last")
REPEAT_FIELDS = (("rec", np.uint32), ("lag", np.uint32), ("lag_lo", np.uint32), ("lag_hi", np.uint32), ("first", np.uint32),
                 ("last", np.uint32), ("pairs", np.uint64), ("cells", np.uint32))


def repeats_fold_raw(cell_off, lag, block, pairs, first, last, lag_tol=1, max_gap=1, min_pairs=100, cap=0, fill=0):
    """One shz_repeats_fold as it is (host only): (rc, repeats, count) with room for `cap` repeats (arrays REPEAT_FIELDS)."""
    co = np.ascontiguousarray(cell_off, np.uint64)
    cols = [np.ascontiguousarray(a, np.uint32) for a in (lag, block, pairs, first, last)]
    assert all(len(a) >= int(co[-1]) for a in cols) if len(co) else True
    rep = {k: np.full(int(cap), fill, d) for k, d in REPEAT_FIELDS}
    cnt = C.c_uint64(fill)
    rc = lib().shz_repeats_fold(ptr(co), len(co) - 1, *[ptr(a) for a in cols], int(lag_tol), int(max_gap), int(min_pairs),
                                *[ptr(rep[k]) if cap else None for k, _ in REPEAT_FIELDS], int(cap), C.byref(cnt))
    return rc, rep, int(cnt.value)


def repeats_fold(cell_off, lag, block, pairs, first, last, lag_tol=1, max_gap=1, min_pairs=100) -> dict:
    """shz_repeats_fold (host only, two calls): the repeat cells of shz_repeats_* joined into repeats -- arrays rec, lag (the
    lag holding the most pairs), lag_lo, lag_hi, first, last (frames: [first, last] airs again at [first + lag, last + lag]),
    pairs, cells; ordered by (rec, first, lag)."""
    args = (cell_off, lag, block, pairs, first, last, lag_tol, max_gap, min_pairs)
    rc, rep, n = repeats_fold_raw(*args, 0)
    if rc == E_CAPACITY:
        rc, rep, n = repeats_fold_raw(*args, n)
    if rc != OK:
        raise ShzError(rc, "shz_repeats_fold: bad arguments")
    return rep


ZONE_FIELDS = ("lo", "hi", "count", "q_first", "q_last", "t_first", "t_last", "shift")


def scan_zones_raw(seg, frames, window_frames, step_frames, margin_frames):
    """One shz_scan_zones as it is (host only): (rc, lo, hi), the zones [n_segs, 3] of the segments seg = the dict of
    scan_timeline (rec, sid, shift, first, last are read)."""
    a = {k: np.ascontiguousarray(seg[k], d) for k, d in SEGMENT_FIELDS[:5]}
    n = len(a["rec"])
    assert all(len(v) == n for v in a.values())
    fr = np.ascontiguousarray(frames, np.uint64)
    lo, hi = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)
    rc = lib().shz_scan_zones(*[ptr(a[k]) for k, _ in SEGMENT_FIELDS[:5]], n, ptr(fr), len(fr), int(window_frames), int(step_frames),
                              int(margin_frames), ptr(lo), ptr(hi))
    return rc, lo, hi


def scan_zones(seg, frames, window_frames, step_frames, margin_frames):
    """shz_scan_zones (host only): the three zones [lo, hi) of recording frames of every segment -- whole, head, tail -- as
    two arrays [n_segs, 3] (include/shz.h at shz_scan_zones)."""
    rc, lo, hi = scan_zones_raw(seg, frames, window_frames, step_frames, margin_frames)
    if rc != OK:
        raise ShzError(rc, "shz_scan_zones: bad arguments")
    return lo, hi


# the segments shz_scan_play_zones / shz_scan_plays read (a warped timeline's, each with its own Q16 pair), and their zone outputs
PLAY_SEGMENT_FIELDS = (("rec", np.uint32), ("sid", np.uint32), ("first", np.uint32), ("last", np.uint32), ("pos_first", np.int32),
                       ("pos_last", np.int32), ("t16", np.uint32), ("f16", np.uint32))
PLAY_ZONE_FIELDS = (("lo", np.uint32), ("hi", np.uint32), ("d_lo", np.int32), ("d_hi", np.int32), ("count", np.uint32),
                    ("q_first", np.uint32), ("q_last", np.uint32), ("t_first", np.uint32), ("t_last", np.uint32),
                    ("shift", np.uint32), ("sum_q", np.uint64), ("sum_u", np.uint64), ("sum_qq", np.uint64), ("sum_qu", np.uint64))


def _play_segments(seg) -> dict:
    a = {k: np.ascontiguousarray(seg[k], d).reshape(-1) for k, d in PLAY_SEGMENT_FIELDS if k in seg}
    if "f16" not in a:
        a["f16"] = a["t16"]
    assert all(len(v) == len(a["rec"]) for v in a.values())
    return a


def scan_play_zones_raw(seg, frames, window_frames, step_frames, margin_frames, w, fill=0):
    """One shz_scan_play_zones as it is (host only): (rc, zones) for the segments seg (rec, sid, first, last, pos_first, pos_last,
    t16 are read); zones = arrays lo, hi (uint32), wlo, whi (uint64), d_lo, d_hi (int32), cand_n (uint32), [n_segs, 3] each,
    filled with `fill` before the call."""
    a = _play_segments(seg)
    n = len(a["rec"])
    fr = np.ascontiguousarray(frames, np.uint64)
    z = {k: np.full((n, 3), fill, d) for k, d in (("lo", np.uint32), ("hi", np.uint32), ("wlo", np.uint64), ("whi", np.uint64),
                                                   ("d_lo", np.int32), ("d_hi", np.int32), ("cand_n", np.uint32))}
    rc = lib().shz_scan_play_zones(*[ptr(a[k]) for k, _ in PLAY_SEGMENT_FIELDS[:7]], n, ptr(fr), len(fr), int(window_frames),
                                   int(step_frames), int(margin_frames), int(w), *[ptr(v) for v in z.values()])
    return rc, z


def scan_play_zones(seg, frames, window_frames, step_frames, margin_frames, w):
    """shz_scan_play_zones (host only): the three zones of every segment of a warped scan -- lo / hi in the
    recording's own frames, wlo / whi warped with the segment's time factor -- and the one widened candidate of every zone
    (d_lo, d_hi; cand_n 0 where it lies outside int32), w = the vote tolerance + drift_bins."""
    rc, z = scan_play_zones_raw(seg, frames, window_frames, step_frames, margin_frames, w)
    if rc != OK:
        raise ShzError(rc, "shz_scan_play_zones: bad segments or factors (INVALID), or a zone of 2^20 warped frames / a candidate "
                           "of 4,096 bins or more (UNSUPPORTED)")
    return z


SPEED_SEGMENT_FIELDS = (("rec", np.uint32), ("sid", np.uint32), ("first", np.uint32), ("last", np.uint32), ("hits", np.uint32),
                        ("best", np.uint32), ("pos_first", np.int32), ("pos_last", np.int32), ("rung", np.uint32))


def scan_timeline_speeds_raw(win_off, sid, delta, aligned, nres, best, step_frames, speeds, min_aligned, max_gap=1, rung_tol=1,
                             shift_tol=2, cap=0):
    """One shz_scan_timeline_speeds as it is (host only): (rc, segments, count) with room for `cap` segments."""
    return _timeline_raw(lib().shz_scan_timeline_speeds, SPEED_SEGMENT_FIELDS, win_off, sid, delta, aligned, nres, step_frames,
                         min_aligned, max_gap, cap, best, (speeds,), (rung_tol, shift_tol))


def scan_timeline_speeds(win_off, sid, delta, aligned, nres, best, step_frames, speeds, min_aligned, max_gap=1, rung_tol=1,
                         shift_tol=2) -> dict:
    """shz_scan_timeline_speeds (host only, two calls): the rank-0 answers of a speed-tolerant scan folded into segments by
    local continuity -- arrays rec, sid, first / last (windows of the recording), hits, best (largest aligned count),
    pos_first / pos_last (song frames at the first / last hit's start), rung (the index chosen most often)."""
    return _timeline(scan_timeline_speeds_raw, "shz_scan_timeline_speeds", win_off, sid, delta, aligned, nres, best, step_frames,
                     speeds, min_aligned, max_gap, rung_tol, shift_tol)


WARP_SEGMENT_FIELDS = SPEED_SEGMENT_FIELDS[:-1] + (("warp", np.uint32),)


def scan_timeline_warps_raw(win_off, sid, delta, aligned, nres, best, step_frames, tempos, pitches, min_aligned, max_gap=1,
                            tempo_tol=0, pitch_tol=0, shift_tol=2, cap=0):
    """One shz_scan_timeline_warps as it is (host only): (rc, segments, count) with room for `cap` segments."""
    return _timeline_raw(lib().shz_scan_timeline_warps, WARP_SEGMENT_FIELDS, win_off, sid, delta, aligned, nres, step_frames,
                         min_aligned, max_gap, cap, best, (tempos, pitches), (tempo_tol, pitch_tol, shift_tol))


def scan_timeline_warps(win_off, sid, delta, aligned, nres, best, step_frames, tempos, pitches, min_aligned, max_gap=1,
                        tempo_tol=0, pitch_tol=0, shift_tol=2) -> dict:
    """shz_scan_timeline_warps (host only, two calls): the rank-0 answers of a scan over warps folded into segments by local
    continuity -- the arrays of scan_timeline_speeds with warp (the variant chosen most often) in place of rung.  tempo_tol /
    pitch_tol: how far the factors of neighbouring hits may lie apart, Q16."""
    return _timeline(scan_timeline_warps_raw, "shz_scan_timeline_warps", win_off, sid, delta, aligned, nres, best, step_frames,
                     tempos, pitches, min_aligned, max_gap, tempo_tol, pitch_tol, shift_tol)


def _floor_into(ctx, res, before, n):
    """The n rows a call recorded, those behind the `before` rows that were in the store, into res as song_hist / bin_hist
    (the store is taken whole: Context.floor() drops what is left over anyway)."""
    sh, bh = ctx.take_floor()
    if len(sh) - before != n:
        raise ShzError(E_STATE, f"vote floor: {len(sh) - before} rows recorded for {n} queries")
    res["song_hist"], res["bin_hist"] = sh[before:], bh[before:]


class Table:
    """HBM-resident fingerprints table: rows (key32, song_id, offset)."""

    def __init__(self, ctx: Context):
        self.ctx, self.h = ctx, None
        h = vp()
        ctx.check(lib().shz_table_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if self.h and self.ctx.h:
            lib().shz_table_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert(self, key32, sid, off):
        k = np.ascontiguousarray(key32, np.uint32)
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sid, np.uint32), k.shape))
        o = np.ascontiguousarray(off, np.uint32)
        assert k.shape == s.shape == o.shape
        self.ctx.check(lib().shz_table_insert(self.h, ptr(k), ptr(s), ptr(o), len(k), 0))

    def insert_clips(self, key32, t1, hash_off, sid0, device=False):
        ho = np.ascontiguousarray(hash_off, np.uint64)
        if not device:
            key32 = np.ascontiguousarray(key32, np.uint32)
            t1 = np.ascontiguousarray(t1, np.uint32)
        self.ctx.check(lib().shz_table_insert_clips(self.h, ptr(key32), ptr(t1), ho.ctypes.data_as(u64p), len(ho) - 1, sid0,
                                                    IN_DEVICE if device else 0))

    def set_segment_rows(self, rows: int):
        self.ctx.check(lib().shz_table_set_segment_rows(self.h, int(rows)))

    def finalize(self):
        self.ctx.check(lib().shz_table_finalize(self.h))

    def reserve(self, rows_hint: int, batch_rows_hint: int = 0, gather: bool = False, wait: bool = False):
        """Announce the size of a bulk build: the table's arenas are allocated once, beside the first batches (wait: before
        this call returns).  gather: the table holds its sealed runs until finalize() / allgather() merges them all at once
        (what a gathered build needs -- every row can still travel -- and what cuts segments by key range)."""
        self.ctx.check(lib().shz_table_reserve(self.h, int(rows_hint), int(batch_rows_hint),
                                               (RESERVE_GATHER if gather else 0) | (RESERVE_WAIT if wait else 0)))

    def seal_run(self):
        """Staged rows -> one sorted run (not yet visible to queries); finalize() merges the runs."""
        self.ctx.check(lib().shz_table_seal_run(self.h))

    def delete_songs(self, sids) -> int:
        """Remove every row of the listed song ids (ON DELETE CASCADE, mysql_database.py:57-58); returns rows removed."""
        a = np.ascontiguousarray(sids, np.uint32)
        n = C.c_uint64()
        self.ctx.check(lib().shz_table_delete_songs(self.h, ptr(a), len(a), C.byref(n)))
        return int(n.value)

    def clear(self):
        self.ctx.check(lib().shz_table_clear(self.h))

    def rows(self):
        a, b = C.c_uint64(), C.c_uint64()
        self.ctx.check(lib().shz_table_rows(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def segments(self) -> int:
        n = C.c_uint32()
        self.ctx.check(lib().shz_table_segments(self.h, C.byref(n)))
        return n.value

    def export(self):
        n, _ = self.rows()
        k, s, o, cnt = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32), C.c_uint64()
        self.ctx.check(lib().shz_table_export(self.h, ptr(k), ptr(s), ptr(o), n, C.byref(cnt)))
        return k, s, o

    def lookup(self, keys):
        """Rows of the listed keys: (key32, sid, off) arrays, grouped in key-list order."""
        kk = np.ascontiguousarray(keys, np.uint32)
        cap = max(1024, 4 * len(kk))
        while True:
            k, s, o, cnt = np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.uint32), C.c_uint64()
            rc = lib().shz_table_lookup(self.h, ptr(kk), len(kk), ptr(k), ptr(s), ptr(o), cap, C.byref(cnt))
            if rc == E_CAPACITY:
                cap = int(cnt.value)
                continue
            self.ctx.check(rc)
            n = int(cnt.value)
            return k[:n], s[:n], o[:n]

    def song_rows(self, sid) -> int:
        n = C.c_uint64()
        self.ctx.check(lib().shz_table_song_rows(self.h, int(sid), C.byref(n)))
        return n.value

    def song_hashes(self, sids, counts_only=False):
        """Rows of the listed songs (shz_table_song_hashes): (row_off, key32, off) -- song sids[i] owns the rows
        [row_off[i], row_off[i + 1]), ordered by (key32, offset).  counts_only: row_off alone is filled (key32 / off come
        back empty), no row is copied."""
        a = np.ascontiguousarray(sids, np.uint32).reshape(-1)
        ro = np.zeros(len(a) + 1, np.uint64)
        empty = np.empty(0, np.uint32)
        self.ctx.check(lib().shz_table_song_hashes(self.h, ptr(a), len(a), ro.ctypes.data_as(u64p), None, None, 0, 0))
        n = int(ro[-1])
        if counts_only or n == 0:
            return ro, empty, empty.copy()
        k, o = np.empty(n, np.uint32), np.empty(n, np.uint32)
        self.ctx.check(lib().shz_table_song_hashes(self.h, ptr(a), len(a), ro.ctypes.data_as(u64p), ptr(k), ptr(o), n, 0))
        return ro, k, o

    def match_songs(self, sids, topn=5, full_sort=False):
        """Every listed song matched against the rest of the table (shz_match_songs): the dict of match(), one query per
        listed song with the song itself left out, plus "rows", the songs' row counts."""
        a = np.ascontiguousarray(sids, np.uint32).reshape(-1)
        res = _match_result(len(a), topn)
        res["rows"] = np.zeros(len(a), np.uint64)
        self.ctx.check(lib().shz_match_songs(self.ctx.h, self.h, ptr(a), len(a), topn, MATCH_FULL_SORT if full_sort else 0,
                                             ptr(res["rows"]), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]),
                                             ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"])))
        return res

    def match_songs_warps(self, sids, tempos, pitches, topn=5, full_sort=False, timings=False):
        """Every listed song at every warp (tempos[v], pitches[v]) matched against the rest of the table
        (shz_match_songs_warps): the dict of match_songs with a warp axis -- sid, delta, aligned, dedup [n, n_warps, topn];
        nres, nhash, npairs [n, n_warps]; rows [n].  timings: the dict also holds "ms" = (gather, warp, match) device times."""
        a = np.ascontiguousarray(sids, np.uint32).reshape(-1)
        tq, fq = np.ascontiguousarray(tempos, np.uint32), np.ascontiguousarray(pitches, np.uint32)
        if tq.shape != fq.shape or tq.ndim != 1:
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        n, K = len(a), len(tq)
        res = {k: v.reshape((n, K) + v.shape[1:]) for k, v in _match_result(n * K, topn).items()}
        res["rows"] = np.zeros(n, np.uint64)
        ms = [C.c_float(), C.c_float(), C.c_float()]
        self.ctx.check(lib().shz_match_songs_warps(self.ctx.h, self.h, ptr(a), n, topn, tq.ctypes.data_as(u32p),
                                                   fq.ctypes.data_as(u32p), K, MATCH_FULL_SORT if full_sort else 0,
                                                   ptr(res["rows"]), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]),
                                                   ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"]),
                                                   *[C.byref(m) if timings else None for m in ms]))
        if timings:
            res["ms"] = tuple(float(m.value) for m in ms)
        return res

    def _extent_args(self, n, cand_sid, d_lo, d_hi, cand_n, hist):
        """the candidate arrays as [n, ncand] (a 1-d list is one slot a query) and the dict of zeroed outputs"""
        cs = np.ascontiguousarray(cand_sid, np.uint32)
        if cs.ndim == 1:
            cs = cs.reshape(n, -1) if n else cs.reshape(0, 1)
        lo = np.ascontiguousarray(d_lo, np.int32).reshape(cs.shape)
        hi = np.ascontiguousarray(d_hi, np.int32).reshape(cs.shape)
        if cs.ndim != 2 or cs.shape[0] != n:
            raise ValueError(f"candidates are [n, ncand] arrays with n = {n}; got {cs.shape}")
        ncand = cs.shape[1]
        cn = (np.full(n, ncand, np.uint32) if cand_n is None else np.ascontiguousarray(cand_n, np.uint32).reshape(-1))
        if len(cn) != n:
            raise ValueError(f"cand_n has {len(cn)} entries for {n} queries")
        res = {k: np.zeros((n, ncand), np.uint32) for k in ("count", "q_first", "q_last", "t_first", "t_last")}
        res["hist"] = np.zeros((n, ncand, 64), np.uint32) if hist else None
        res["shift"] = np.zeros(n, np.uint32)
        return cs, lo, hi, cn, ncand, res

    def match_extents(self, key32, q_off, query_off, cand_sid, d_lo, d_hi, cand_n=None, hist=True, fit=False):
        """Where the aligned hashes lie (shz_match_extents): per query and candidate (song cand_sid, offset differences d_lo ..
        d_hi inclusive) the pairs that belong -- count, q_first / q_last (query frames), t_first / t_last (song frames) as
        [n, ncand], hist [n, ncand, 64] (pairs per bucket q_off >> shift; None with hist false), shift [n].  Candidates are
        [n, ncand] arrays, of which query q uses the first cand_n[q] (None: all); everything past them is zero.
        fit (shz_match_extents_fit): the moments of every candidate's pairs too -- sum_q, sum_u, sum_qq, sum_qu [n, ncand]
        (uint64, modulo 2^64) with q = q_off and u = (off - q_off) - d_lo; a used candidate must span less than 4,096 bins.
        The key cap is taken from the context: inside `with ctx.key_cap(rows):` every output covers the kept pairs only."""
        k = np.ascontiguousarray(key32, np.uint32)
        o = np.ascontiguousarray(q_off, np.uint32)
        qo = np.ascontiguousarray(query_off, np.uint64)
        n = len(qo) - 1
        cs, lo, hi, cn, ncand, res = self._extent_args(n, cand_sid, d_lo, d_hi, cand_n, hist)
        if fit:
            sums = {f: np.zeros((n, ncand), np.uint64) for f in ("sum_q", "sum_u", "sum_qq", "sum_qu")}
            self.ctx.check(lib().shz_match_extents_fit(self.ctx.h, self.h, ptr(k), ptr(o), qo.ctypes.data_as(u64p), n, ncand, ptr(cs),
                                                       ptr(lo), ptr(hi), ptr(cn), ptr(res["count"]), ptr(res["q_first"]),
                                                       ptr(res["q_last"]), ptr(res["t_first"]), ptr(res["t_last"]),
                                                       ptr(res["hist"]), ptr(res["shift"]), *[ptr(a) for a in sums.values()]))
            res.update(sums)
            return res
        self.ctx.check(lib().shz_match_extents(self.ctx.h, self.h, ptr(k), ptr(o), qo.ctypes.data_as(u64p), n, ncand, ptr(cs),
                                               ptr(lo), ptr(hi), ptr(cn), ptr(res["count"]), ptr(res["q_first"]),
                                               ptr(res["q_last"]), ptr(res["t_first"]), ptr(res["t_last"]), ptr(res["hist"]),
                                               ptr(res["shift"])))
        return res

    def match_songs_extents(self, sids, cand_sid, d_lo, d_hi, cand_n=None, hist=True):
        """match_extents with the listed songs' own rows as the queries (shz_match_songs_extents): the rows are gathered on the
        device; q_first / q_last are offsets of the listed song, t_first / t_last of the candidate song."""
        a = np.ascontiguousarray(sids, np.uint32).reshape(-1)
        n = len(a)
        cs, lo, hi, cn, ncand, res = self._extent_args(n, cand_sid, d_lo, d_hi, cand_n, hist)
        self.ctx.check(lib().shz_match_songs_extents(self.ctx.h, self.h, ptr(a), n, ncand, ptr(cs), ptr(lo), ptr(hi), ptr(cn),
                                                     ptr(res["count"]), ptr(res["q_first"]), ptr(res["q_last"]),
                                                     ptr(res["t_first"]), ptr(res["t_last"]), ptr(res["hist"]),
                                                     ptr(res["shift"])))
        return res

    def match_songs_warps_extents(self, job_sid, tempos, pitches, cand_sid, d_lo, d_hi, cand_n=None, hist=False, timings=False):
        """match_extents(..., fit=True) with songs of the table, warped on the device, as the queries
        (shz_match_songs_warps_extents): job j is song job_sid[j] under the row warp (tempos[j], pitches[j]) (Q16); one song
        may stand in several jobs.  Returns the dict of match_extents(..., fit=True) over the jobs -- q_first / q_last are
        WARPED frames of the listed song (extent.own_frames takes them back), t_first / t_last frames of the candidate song --
        plus "kept" [n], the kept warped rows of every job before rows that meet in one (key, t1') collapse.  timings: the
        dict also holds "ms" = (gather, warp, extent) device times."""
        a = np.ascontiguousarray(job_sid, np.uint32).reshape(-1)
        tq, fq = np.ascontiguousarray(tempos, np.uint32).reshape(-1), np.ascontiguousarray(pitches, np.uint32).reshape(-1)
        n = len(a)
        if len(tq) != n or len(fq) != n:
            raise ValueError("job_sid, tempos and pitches are three lists of one length: job j is (job_sid[j], tempos[j], pitches[j])")
        cs, lo, hi, cn, ncand, res = self._extent_args(n, cand_sid, d_lo, d_hi, cand_n, hist)
        sums = {f: np.zeros((n, ncand), np.uint64) for f in ("sum_q", "sum_u", "sum_qq", "sum_qu")}
        kept = np.zeros(n, np.uint64)
        ms = [C.c_float(), C.c_float(), C.c_float()]
        self.ctx.check(lib().shz_match_songs_warps_extents(
            self.ctx.h, self.h, a.ctypes.data_as(u32p), tq.ctypes.data_as(u32p), fq.ctypes.data_as(u32p), n, ncand, ptr(cs), ptr(lo),
            ptr(hi), ptr(cn), ptr(res["count"]), ptr(res["q_first"]), ptr(res["q_last"]), ptr(res["t_first"]), ptr(res["t_last"]),
            ptr(res["hist"]), ptr(res["shift"]), *[ptr(s) for s in sums.values()], ptr(kept),
            *[C.byref(m) if timings else None for m in ms]))
        res.update(sums)
        res["kept"] = kept
        if timings:
            res["ms"] = tuple(float(m.value) for m in ms)
        return res

    def finalize_runs(self, run_rows):
        """finalize() for staged rows that are consecutive blocks of run_rows[r] rows: every block is sorted on its own
        and the sorted runs are merged -- what allgather() does with the ranks' rows, without a communicator."""
        rr = np.ascontiguousarray(run_rows, np.uint64)
        self.ctx.check(lib().shz_table_finalize_runs(self.h, rr.ctypes.data_as(u64p), len(rr)))

    def build_stats(self) -> dict:
        v = [C.c_double() for _ in range(4)]
        self.ctx.check(lib().shz_table_build_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("sort_s", "exchange_s", "merge_s", "segments_s"), (float(x.value) for x in v)))

    def phase_stats(self, reset=False) -> dict:
        """Host seconds per build phase since the last reset (shz_table_phase_stats)."""
        n = C.c_uint32()
        self.ctx.check(lib().shz_table_phase_stats(self.h, None, 0, C.byref(n), 0))
        v = (C.c_double * n.value)()
        self.ctx.check(lib().shz_table_phase_stats(self.h, v, n.value, C.byref(n), 1 if reset else 0))
        return {lib().shz_table_phase_name(i).decode(): float(v[i]) for i in range(n.value)}

    def set_run_rows(self, rows: int):
        """Rows one sealed run may hold (0: 2^32 - 4096); small values force many runs (tests)."""
        self.ctx.check(lib().shz_table_set_run_rows(self.h, int(rows)))

    def exchange_run(self, comm: "Comm"):
        """Collective: seal the staged rows and start this round's runs travelling to every peer on the communicator's own
        stream; returns with the transfers in flight (the next batch is fingerprinted beside them)."""
        self.ctx.check(lib().shz_table_exchange_run(self.h, comm.h))

    def exchange_stats(self) -> dict:
        r, b, w, k = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_uint32()
        self.ctx.check(lib().shz_table_exchange_stats(self.h, C.byref(r), C.byref(b), C.byref(w), C.byref(k)))
        return {"rounds": r.value, "bytes_received": b.value, "wait_s": w.value, "runs_held": k.value}

    def allgather(self, comm: "Comm") -> int:
        """Collective: seal what is staged, exchange every run not yet sent, merge all runs into the node-global table;
        returns the payload bytes this rank received."""
        b = C.c_uint64()
        self.ctx.check(lib().shz_table_allgather(self.h, comm.h, C.byref(b)))
        return b.value

    def _filter_of(self, nq, songs, exclude, song_sets, set_of):
        """the arguments of Context.songs() for a match call, and the uint32 map of its queries (None: set 0)"""
        if (song_sets is None) != (set_of is None):
            raise ValueError("song_sets= and set_of= go together")
        if song_sets is not None and (songs is not None or (exclude is not None and not isinstance(exclude, bool))):
            raise ValueError("song_sets= goes without songs= and without an exclude= list (exclude=True bars the listed songs)")
        if song_sets is None:
            return dict(only=songs, exclude=exclude), None
        m = np.ascontiguousarray(set_of, np.uint32).reshape(-1)
        if len(m) != nq:
            raise ValueError(f"set_of has {len(m)} entries for {nq} queries")
        return dict(sets=list(song_sets), exclude=bool(exclude)), m

    def match(self, key32, q_off, query_off, topn=2, full_sort=False, delta_tol=None, floor=False, songs=None, exclude=None,
              song_sets=None, set_of=None, max_key_rows=None):
        """Batched return_matches + align_matches.  Returns dict of arrays (see shz.h).  full_sort: the vote as one
        sort of 8-byte votes + record chain (SHZ_MATCH_FULL_SORT), the form the faster vote paths are tested against.
        delta_tol: the vote tolerance of this call (Context.tolerance); None: the context's.  floor: the result gains
        song_hist and bin_hist, [n_queries, 32] uint32 (Context.floor, shazam_amd.floor); the other arrays do not change.  Rows
        that a context with the floor switched on by hand had recorded before are dropped (Context.floor).
        songs= / exclude= (song ids): the match within / without these songs, one set for all queries (Context.songs; the
        arrays of a plain match on a table of the allowed songs' rows only; npairs counts the kept pairs).  song_sets= (a
        list of id lists) with set_of= (a set index per query): per-query sets (shz_match_batch_sets); exclude=True bars
        the listed songs.  The context's own filter is back in force afterwards.
        max_key_rows: the key cap of this call (Context.key_cap: keys that hold more table rows vote for nobody; the arrays
        of a plain match on a table lacking those keys' rows; 0: off); None: the context's."""
        k = np.ascontiguousarray(key32, np.uint32)
        o = np.ascontiguousarray(q_off, np.uint32)
        qo = np.ascontiguousarray(query_off, np.uint64)
        nq = len(qo) - 1
        res = _match_result(nq, topn)
        filt, smap = self._filter_of(nq, songs, exclude, song_sets, set_of)
        with self.ctx.tolerance(delta_tol), self.ctx.floor(floor), self.ctx.songs(**filt), self.ctx.key_cap(max_key_rows):
            before = self.ctx.floor_rows() if floor else 0
            args = (self.ctx.h, self.h, ptr(k), ptr(o), qo.ctypes.data_as(u64p), nq, topn, MATCH_FULL_SORT if full_sort else 0,
                    ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]), ptr(res["nres"]), ptr(res["nhash"]),
                    ptr(res["npairs"]))
            if smap is None:
                self.ctx.check(lib().shz_match_batch(*args))
            else:
                self.ctx.check(lib().shz_match_batch_sets(*args, ptr(smap)))
            if floor:
                _floor_into(self.ctx, res, before, nq)
        return res

    def match_device(self, key32, q_off, query_off, topn=2, full_sort=False, bias_bound=-1, floor=False, songs=None, exclude=None,
                     song_sets=None, set_of=None, delta_tol=None, max_key_rows=None):
        """match() the way the fused calls and the listeners run it (shz_match_device_host): the two columns are put on the
        device first and matched there, with the caller's bound of the query offsets (below 0 or >= 2^32: none).  For tests
        and tools; same result arrays as match() (floor, songs, exclude, song_sets, set_of, delta_tol, max_key_rows: as
        there)."""
        k = np.ascontiguousarray(key32, np.uint32)
        o = np.ascontiguousarray(q_off, np.uint32)
        qo = np.ascontiguousarray(query_off, np.uint64)
        nq = len(qo) - 1
        res = _match_result(nq, topn)
        filt, smap = self._filter_of(nq, songs, exclude, song_sets, set_of)
        with self.ctx.tolerance(delta_tol), self.ctx.floor(floor), self.ctx.songs(**filt), self.ctx.key_cap(max_key_rows):
            before = self.ctx.floor_rows() if floor else 0
            args = (self.ctx.h, self.h, ptr(k), ptr(o), qo.ctypes.data_as(u64p), nq, topn, MATCH_FULL_SORT if full_sort else 0,
                    int(bias_bound), ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]), ptr(res["nres"]),
                    ptr(res["nhash"]), ptr(res["npairs"]))
            if smap is None:
                self.ctx.check(lib().shz_match_device_host(*args))
            else:
                self.ctx.check(lib().shz_match_device_host_sets(*args, ptr(smap)))
            if floor:
                _floor_into(self.ctx, res, before, nq)
        return res

    def key_hist(self) -> dict:
        """The key sizes of the finalized rows (shz_table_key_hist): {"keys": uint64[32] -- the distinct keys whose row count
        falls into each bucket of shazam_amd.floor.bucket_of (1 .. 16 exact, then powers of two) --, "rows": uint64[32] --
        the rows they hold --, "max_rows": the largest key, "n_keys": the distinct keys}.  shazam_amd.keycap turns it into
        a cap (Context.key_cap)."""
        keys, rows, mx, nk = np.zeros(32, np.uint64), np.zeros(32, np.uint64), C.c_uint64(), C.c_uint64()
        self.ctx.check(lib().shz_table_key_hist(self.h, ptr(keys), ptr(rows), C.byref(mx), C.byref(nk)))
        return {"keys": keys, "rows": rows, "max_rows": int(mx.value), "n_keys": int(nk.value)}

    def match_stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx.check(lib().shz_match_stats(self.ctx.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"rows_scanned": a.value, "pairs": b.value, "distinct_keys": c.value}


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * 128)()
    rc = lib().shz_comm_unique_id(buf)
    if rc != OK:
        raise ShzError(rc, "shz_comm_unique_id failed (librccl.so not loadable?)")
    return bytes(buf)


class Comm:
    """RCCL communicator, one rank per GPU."""

    def __init__(self, ctx: Context, unique_id: bytes, rank: int, nranks: int):
        self.ctx, self.h = ctx, None
        assert len(unique_id) == 128
        idb = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        h = vp()
        ctx.check(lib().shz_comm_create(ctx.h, idb, rank, nranks, C.byref(h)))
        self.h, self.rank, self.nranks = h, rank, nranks

    @classmethod
    def local(cls, ctx: Context, group_id: int, rank: int, nranks: int) -> "Comm":
        """Ranks = threads of this process (one Context each): rendezvous + device copies instead of RCCL."""
        self = cls.__new__(cls)
        self.ctx, self.h = ctx, None
        h = vp()
        ctx.check(lib().shz_comm_create_local(ctx.h, int(group_id), rank, nranks, C.byref(h)))
        self.h, self.rank, self.nranks = h, rank, nranks
        return self

    def warmup(self):
        """Collective: the connections between every pair of ranks exist afterwards (RCCL makes them on first use)."""
        self.ctx.check(lib().shz_comm_warmup(self.h))

    def barrier(self):
        self.ctx.check(lib().shz_comm_barrier(self.h))

    def close(self):
        if self.h and self.ctx.h:
            lib().shz_comm_destroy(self.h)
        self.h = None


def stream_plan(samples_before: int, samples_after: int, settled_before: int, hop: int = HOP, ending: bool = False):
    """shz_stream_plan (host only): (win_frame0, win_s0, win_s1, settled_after) of one push of a stream."""
    v = [C.c_uint64() for _ in range(4)]
    rc = lib().shz_stream_plan(int(samples_before), int(samples_after), int(settled_before), int(hop), 1 if ending else 0,
                               *[C.byref(x) for x in v])
    if rc != OK:
        raise ShzError(rc, "shz_stream_plan: invalid arguments")
    return tuple(int(x.value) for x in v)


class Streams:
    """n independent live streams on one context (shz_streams_*): push chunks, get the hashes that became final."""

    def __init__(self, ctx: Context, n_streams: int, fs: int = 44100, amp_min: float = 10.0, fan_value: int = 5):
        self.ctx, self.h, self.n = ctx, None, int(n_streams)
        h = vp()
        ctx.check(lib().shz_streams_create(ctx.h, self.n, int(fs), float(amp_min), int(fan_value), C.byref(h)))
        self.h, self.fan_value = h, int(fan_value)
        self.hop = int(getattr(ctx, "hop", HOP))
        self.cap = 4096

    def close(self):
        if self.h and self.ctx.h:
            lib().shz_streams_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _end_bits(self, end):
        if end is None:
            return None
        words = np.zeros((self.n + 31) // 32, np.uint32)
        for i in (range(self.n) if end is True else end):
            words[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))
        return words

    def push_raw(self, pcm, chunk_off, end=None, cap=None, pcm_device=False, out_key: DevBuf = None, out_t1: DevBuf = None):
        """One shz_streams_push as it is: returns (rc, key32, t1, hash_off, count) without retrying."""
        co = np.ascontiguousarray(chunk_off, np.uint64)
        assert len(co) == self.n + 1
        ew = self._end_bits(end)
        ho, cnt = np.zeros(self.n + 1, np.uint64), C.c_uint64()
        flags = PCM_DEVICE if pcm_device else 0
        if out_key is not None:
            cap = int(cap if cap is not None else out_key.nbytes // 4)
            rc = lib().shz_streams_push(self.h, ptr(pcm), co.ctypes.data_as(u64p), ptr(ew), flags | OUT_DEVICE, ptr(out_key),
                                        ptr(out_t1), ho.ctypes.data_as(u64p), cap, C.byref(cnt))
            return rc, None, None, ho, int(cnt.value)
        cap = int(self.cap if cap is None else cap)
        k, t1 = np.empty(max(cap, 1), np.uint32), np.empty(max(cap, 1), np.uint32)
        rc = lib().shz_streams_push(self.h, ptr(pcm), co.ctypes.data_as(u64p), ptr(ew), flags, ptr(k), ptr(t1),
                                    ho.ctypes.data_as(u64p), cap, C.byref(cnt))
        n = int(cnt.value)
        return rc, k[:n], t1[:n], ho, n

    def push(self, chunks, end=None):
        """chunks: one 1-D int16 array per stream (None / empty: nothing for it).  end: stream indices that end after this
        chunk (True: all).  Returns (key32, t1, hash_off) of the hashes that became final, stream i's at
        [hash_off[i], hash_off[i+1]); retries with the required capacity on E_CAPACITY like Context.fingerprint_batch."""
        assert len(chunks) == self.n
        arrs = [np.zeros(0, np.int16) if c is None else np.ascontiguousarray(c, np.int16) for c in chunks]
        off = np.zeros(self.n + 1, np.uint64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)
        while True:
            rc, k, t1, ho, n = self.push_raw(pcm, off, end)
            if rc == E_CAPACITY:
                self.cap = max(n, 2 * self.cap)
                continue
            self.ctx.check(rc)
            return k.copy(), t1.copy(), ho

    def reset(self, which=None):
        """Start streams afresh (default: all of them)."""
        w = np.ascontiguousarray(range(self.n) if which is None else which, np.uint32)
        self.ctx.check(lib().shz_streams_reset(self.h, ptr(w), len(w)))

    def state(self, i: int) -> dict:
        v = [C.c_uint64() for _ in range(4)]
        self.ctx.check(lib().shz_streams_state(self.h, int(i), *[C.byref(x) for x in v]))
        return dict(zip(("samples", "settled", "pending", "emitted"), (int(x.value) for x in v)))


def listener_window(settled, window_frames: int):
    """shz_listener_window (host only): (H, w0) of a listener whose channels have settled[c] frames."""
    st = np.ascontiguousarray(settled, np.uint64)
    h, w0 = C.c_uint64(), C.c_uint64()
    rc = lib().shz_listener_window(st.ctypes.data_as(u64p), len(st), int(window_frames), C.byref(h), C.byref(w0))
    if rc != OK:
        raise ShzError(rc, "shz_listener_window: invalid arguments")
    return int(h.value), int(w0.value)


class Listeners:
    """Device-resident listeners over a Streams object and a Table (shz_listeners_*): listener l = the adjacent streams
    [l channels, (l + 1) channels); its window of settled hashes stays on the device between pushes.  peaks=True
    (shz_listeners_create_peaks): the windows hold settled PEAKS per channel, and the pushes are push_warps / push_speeds --
    every listener at every variant of a ladder; push / window are SHZ_E_STATE on it, as push_warps / push_speeds / peaks
    are without it."""

    def __init__(self, streams: Streams, table: Table, n_listeners: int, window_frames: int, peaks: bool = False):
        self.ctx, self.streams, self.table, self.h, self.n = streams.ctx, streams, table, None, int(n_listeners)
        self.peak_windows = bool(peaks)
        h = vp()
        create = lib().shz_listeners_create_peaks if peaks else lib().shz_listeners_create
        self.ctx.check(create(streams.h, table.h, self.n, int(window_frames), C.byref(h)))
        self.h = h

    def close(self):
        if self.h and self.ctx.h and self.streams.h:
            lib().shz_listeners_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push_raw(self, pcm, chunk_off, end=None, topn=2, pcm_device=False, full_sort=False):
        """One shz_listeners_push as it is: (rc, res, w0) with res as Table.match over the listeners."""
        co = np.ascontiguousarray(chunk_off, np.uint64)
        assert len(co) == self.streams.n + 1
        ew = self.streams._end_bits(end)
        res, w0 = _match_result(self.n, topn), np.zeros(self.n, np.uint32)
        rc = lib().shz_listeners_push(self.h, ptr(pcm), co.ctypes.data_as(u64p), ptr(ew), int(topn),
                                      (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0),
                                      ptr(res["sid"]), ptr(res["delta"]), ptr(res["aligned"]), ptr(res["dedup"]),
                                      ptr(res["nres"]), ptr(res["nhash"]), ptr(res["npairs"]), ptr(w0))
        return rc, res, w0

    def push(self, chunks, end=None, topn=2):
        """chunks: one 1-D int16 array per STREAM (None / empty: nothing for it); end: stream indices that end after this
        chunk.  Returns (res, w0)."""
        assert len(chunks) == self.streams.n
        arrs = [np.zeros(0, np.int16) if c is None else np.ascontiguousarray(c, np.int16) for c in chunks]
        off = np.zeros(self.streams.n + 1, np.uint64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)
        rc, res, w0 = self.push_raw(pcm, off, end, topn)
        self.ctx.check(rc)
        return res, w0

    def reset(self, which=None):
        w = np.ascontiguousarray(range(self.n) if which is None else which, np.uint32)
        self.ctx.check(lib().shz_listeners_reset(self.h, ptr(w), len(w)))

    def state(self, l: int) -> dict:
        a, b = C.c_uint64(), C.c_uint64()
        self.ctx.check(lib().shz_listeners_state(self.h, int(l), C.byref(a), C.byref(b)))
        return {"window_hashes": int(a.value), "w0": int(b.value)}

    def window(self, l: int):
        """(key32, t1, q_off) of listener l's window, in the order the device keeps them (shz_listeners_window); q_off is what
        the last push handed to the match.  For tests and tools."""
        n = C.c_uint64()
        rc = lib().shz_listeners_window(self.h, int(l), None, None, None, 0, C.byref(n))
        if rc != E_CAPACITY:
            self.ctx.check(rc)
        cnt = int(n.value)
        k, t, q = (np.zeros(cnt, np.uint32) for _ in range(3))
        if cnt:
            self.ctx.check(lib().shz_listeners_window(self.h, int(l), ptr(k), ptr(t), ptr(q), cnt, C.byref(n)))
        return k, t, q

    def _cat(self, chunks):
        assert len(chunks) == self.streams.n
        arrs = [np.zeros(0, np.int16) if c is None else np.ascontiguousarray(c, np.int16) for c in chunks]
        off = np.zeros(self.streams.n + 1, np.uint64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        return (np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)), off

    def push_warps_raw(self, pcm, chunk_off, tempos, pitches=None, end=None, topn=2, pcm_device=False, full_sort=False):
        """One shz_listeners_push_warps as it is (pitches=None: shz_listeners_push_speeds with the ladder `tempos`): (rc, res,
        w0) with res as Context.recognize_warps' over the listeners -- the best variant's rows, best [n] and profile
        [n, n_warps].  tempos / pitches: Q16."""
        co = np.ascontiguousarray(chunk_off, np.uint64)
        assert len(co) == self.streams.n + 1
        ew = self.streams._end_bits(end)
        tq = np.ascontiguousarray(tempos, np.uint32)
        fq = None if pitches is None else np.ascontiguousarray(pitches, np.uint32)
        if tq.ndim != 1 or (fq is not None and fq.shape != tq.shape):
            raise ValueError("tempos and pitches are two lists of one length: warp v is (tempos[v], pitches[v])")
        res, w0 = _match_result(self.n, topn), np.zeros(self.n, np.uint32)
        del res["npairs"]
        res["best"], res["profile"] = np.zeros(self.n, np.uint32), np.zeros((self.n, len(tq)), np.uint32)
        flags = (PCM_DEVICE if pcm_device else 0) | (MATCH_FULL_SORT if full_sort else 0)
        outs = [ptr(res[k]) for k in ("best", "sid", "delta", "aligned", "dedup", "nres", "nhash", "profile")] + [ptr(w0)]
        if fq is None:
            rc = lib().shz_listeners_push_speeds(self.h, ptr(pcm), co.ctypes.data_as(u64p), ptr(ew), int(topn), ptr(tq), len(tq),
                                                 flags, *outs)
        else:
            rc = lib().shz_listeners_push_warps(self.h, ptr(pcm), co.ctypes.data_as(u64p), ptr(ew), int(topn), ptr(tq), ptr(fq),
                                                len(tq), flags, *outs)
        return rc, res, w0

    def push_warps(self, chunks, tempo, pitch, end=None, topn=2):
        """chunks / end as for push; warp v is (tempo[v], pitch[v]), Q16.  Returns (res, w0)."""
        pcm, off = self._cat(chunks)
        rc, res, w0 = self.push_warps_raw(pcm, off, tempo, pitch, end, topn)
        self.ctx.check(rc)
        return res, w0

    def push_speeds(self, chunks, ladder, end=None, topn=2):
        """push_warps at a speed ladder: the one Q16 table for time and frequency.  Returns (res, w0)."""
        pcm, off = self._cat(chunks)
        rc, res, w0 = self.push_warps_raw(pcm, off, ladder, None, end, topn)
        self.ctx.check(rc)
        return res, w0

    def peaks(self, l: int, channel: int = 0):
        """(f, t) of the peak window of channel `channel` of listener l, t in absolute frames of the stream, in the order the
        device keeps them (shz_listeners_peaks).  For tests and tools."""
        n = C.c_uint64()
        rc = lib().shz_listeners_peaks(self.h, int(l), int(channel), None, None, 0, C.byref(n))
        if rc != E_CAPACITY:
            self.ctx.check(rc)
        cnt = int(n.value)
        f, t = np.zeros(cnt, np.uint16), np.zeros(cnt, np.uint32)
        if cnt:
            self.ctx.check(lib().shz_listeners_peaks(self.h, int(l), int(channel), ptr(f), ptr(t), cnt, C.byref(n)))
        return f, t

    def timing(self, enable: bool = True):
        """(streams, window, warp, match) ms of the last timed push_warps / push_speeds; pushes from now on are timed or
        not (shz_listeners_timing).  For tools."""
        ms = (C.c_float * 4)()
        self.ctx.check(lib().shz_listeners_timing(self.h, 1 if enable else 0, ms))
        return tuple(float(x) for x in ms)
