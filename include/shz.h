/*
 * shz.h -- C ABI of libshz.so, the MI355X (gfx950) fingerprint / match hot path.
 *
 * The reference (CarlosArturoMe/shazam) is pure Python and has no FFI of its own
 * (SURVEY.md 8b); this header is the boundary a maintainer binds with ctypes to put
 * the HIP path behind the reference's own functions.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - every function returns an int32 status: SHZ_OK or a negative SHZ_E_* code;
 *     shz_last_error(ctx) gives a message owned by the ctx (valid until the next call).
 *   - shz_ctx is one (device, stream); NOT thread-safe per ctx, independent ctxs are.
 *   - the caller allocates every output buffer and passes its capacity; on overflow the
 *     call returns SHZ_E_CAPACITY with the required count in *count (two-call idiom).
 *   - pointers are host pointers unless the matching SHZ_*_DEVICE flag is set, in which
 *     case they are device pointers obtained from shz_dev_alloc on the same ctx.
 *   - the library never keeps a caller pointer past return; no exception crosses the ABI.
 */
#ifndef SHZ_H
#define SHZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHZ_OK 0
#define SHZ_E_INVALID (-1)   /* bad argument                                   */
#define SHZ_E_HIP (-2)       /* a HIP runtime call failed                      */
#define SHZ_E_CAPACITY (-3)  /* output buffer too small; *count = required     */
#define SHZ_E_NOMEM (-4)     /* device or host allocation failed               */
#define SHZ_E_UNSUPPORTED (-5)/* parameter combination the HIP path does not implement */
#define SHZ_E_RCCL (-6)      /* RCCL missing or a collective failed            */
#define SHZ_E_STATE (-7)     /* object used in the wrong state                 */

#define SHZ_PCM_DEVICE 1u    /* pcm pointer is device memory                   */
#define SHZ_OUT_DEVICE 2u    /* output pointers are device memory              */
#define SHZ_IN_DEVICE 4u     /* generic: input arrays are device memory        */
#define SHZ_STFT_POWER 8u    /* shz_stft_db: write the PSD itself, not 10*log10 */
#define SHZ_RESERVE_GATHER 32u /* shz_table_reserve: size the run arena for an all-gathered build (every rank's rows) */
#define SHZ_RESERVE_WAIT 64u   /* shz_table_reserve: return when the allocations exist (setup outside a timed region) */
#define SHZ_SCAN_KEEP_MASK 128u /* shz_scan_extents: out_nres holds, on entry, a keep mask of the windows (see there) */
#define SHZ_MATCH_FULL_SORT 16u /* shz_match_batch: 8-byte votes, full radix sort and record chain (the reference form of
                                  the vote: what the 4-byte votes and the vote tiles must reproduce) */

/* constants of the algorithm: __init__.py:41-51 == recognizer.py:21-38 */
#define SHZ_NFFT 4096
#define SHZ_HOP 2048
#define SHZ_NBINS 2049
#define SHZ_PEAK_RADIUS 10
#define SHZ_MAX_DT 200
#define SHZ_DEFAULT_FS 44100

typedef struct shz_ctx shz_ctx;
typedef struct shz_table shz_table;
typedef struct shz_comm shz_comm;

/* ---- context, memory, timing ------------------------------------------------------ */
int32_t shz_ctx_create(int32_t device_id, shz_ctx** out);
int32_t shz_ctx_destroy(shz_ctx* ctx);
const char* shz_last_error(shz_ctx* ctx);
const char* shz_version(void);
/* name: >=128 bytes; any out pointer may be NULL */
int32_t shz_device_info(shz_ctx* ctx, char* name, uint64_t name_cap, uint64_t* hbm_bytes,
                        int32_t* compute_units, int32_t* clock_khz);
/* device memory free / total right now (hipMemGetInfo): sizes reservations, shows leaks in tests */
int32_t shz_mem_info(shz_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
int32_t shz_dev_alloc(shz_ctx* ctx, uint64_t bytes, void** dptr);
int32_t shz_dev_free(shz_ctx* ctx, void* dptr);
int32_t shz_copy_h2d(shz_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);
int32_t shz_copy_d2h(shz_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);
int32_t shz_sync(shz_ctx* ctx);
/* cap on the internal scratch arena (dB spectrogram, masks, sort buffers); batches are
 * split into sub-batches that fit.  0 = default (1/4 of HBM). */
int32_t shz_set_workspace_limit(shz_ctx* ctx, uint64_t bytes);
/* free the scratch arena (it regrows on demand); *freed_bytes may be NULL */
int32_t shz_release_workspace(shz_ctx* ctx, uint64_t* freed_bytes);
/* hipEvent timers on the ctx stream (replaces the time() deltas at recognizer.py:214-220,
 * 282-284, 388-390).  slot in [0,16). */
int32_t shz_timer_start(shz_ctx* ctx, int32_t slot);
int32_t shz_timer_stop(shz_ctx* ctx, int32_t slot, float* elapsed_ms);
/* per-kernel accumulated device time of the last profiled call (see shz_set_profiling).
 * which: 0 stft_psd, 1 peak_pick, 2 peak_expand(+scan), 3 pair_hash(+scan), 4 peak_verify, 5 resample */
int32_t shz_set_profiling(shz_ctx* ctx, int32_t enabled);
int32_t shz_get_kernel_ms(shz_ctx* ctx, int32_t which, float* total_ms, uint32_t* launches);

/* ---- synthetic PCM (bench / tests input; numpy twin: oracle/synth.py) ------------------ */
/* clips [clip0, clip0+n_clips) x n_samples int16, clip-major, written to DEVICE memory.
 * tone_amp = 0 -> white noise uniform in [-noise_amp, noise_amp). */
int32_t shz_synth_pcm(shz_ctx* ctx, uint64_t seed, uint64_t clip0, uint32_t n_clips, uint64_t n_samples,
                      int32_t tone_amp, int32_t noise_amp, uint64_t start_sample, int16_t* dev_out);
/* Music-like tracks (kind SHZ_CORPUS_MUSIC: four voices of decaying harmonic notes, percussive onsets, a quiet noise bed:
 * amp, bed, burst) and traffic-like low-passed noise (SHZ_CORPUS_TRAFFIC: amp) -- stand-ins for what the reference's
 * accuracy figures were measured on (real music under street noise, recognizer_test.py:39-40, 542-558), integer-only with
 * numpy twins (oracle/synth.py: music_clip, traffic_noise).  Same addressing as shz_synth_pcm. */
#define SHZ_CORPUS_MUSIC 1u
#define SHZ_CORPUS_TRAFFIC 2u
int32_t shz_synth_corpus(shz_ctx* ctx, uint32_t kind, uint64_t seed, uint64_t clip0, uint32_t n_clips, uint64_t n_samples,
                         int32_t amp, int32_t bed, int32_t burst, uint64_t start_sample, int16_t* dev_out);

/* HBM bandwidth probe (the measured ceiling beside the vendor peak): mode 0 copy (bytes read +
 * bytes written are counted), 1 read only, 2 write only; two scratch buffers of `bytes` each are allocated and
 * freed inside; gb_per_s = bytes moved / hipEvent time over `iters` launches (16 B per lane, grid-stride).
 * Host link probe (what a host-fed fingerprint call can reach at best): mode 3 pinned host -> device, 4 pageable host ->
 * device, 5 device -> pinned host; `iters` copies of `bytes`, host clock around them. */
int32_t shz_membw(shz_ctx* ctx, int32_t mode, uint64_t bytes, uint32_t iters, float* gb_per_s);

/* The device radix sort the table build and the vote use (tests / tools): stable sort of n 64-bit keys on bits
 * [bit_lo, bit_hi) (other bits are not compared), carrying a payload of val_bytes = 0, 4 or 8
 * bytes per key.  keys / vals are HOST arrays, sorted in place.  n < 2^32. */
int32_t shz_sort_pairs(shz_ctx* ctx, uint64_t* keys, void* vals, uint32_t val_bytes, uint64_t n, uint32_t bit_lo,
                       uint32_t bit_hi);
/* The 4-byte form the vote uses when a pass's query index, song id and offset delta fit 31 bits (tests / tools): stable
 * sort of n 32-bit keys on bits [bit_lo, bit_hi), written as 64-bit keys `key + add` (the last pass widens).
 * keys / out64 are HOST arrays.  n < 2^32. */
int32_t shz_sort_keys32(shz_ctx* ctx, const uint32_t* keys, uint64_t n, uint32_t bit_lo, uint32_t bit_hi, uint64_t add,
                        uint64_t* out64);

/* The SEGMENTED form behind the vote passes (tests / tools): segment i = keys [seg_off[i], seg_off[i+1]), n_segs <= 128;
 * every segment is ordered (stably) among its own keys on bits [bit_lo, bit_hi), no key leaves its segment.
 * keys / seg_off / out are HOST arrays; seg_off[0] = 0, seg_off[n_segs] = n < 2^32. */
int32_t shz_sort_keys32_seg(shz_ctx* ctx, const uint32_t* keys, const uint64_t* seg_off, uint32_t n_segs, uint32_t bit_lo,
                            uint32_t bit_hi, uint32_t* out);

/* The device exclusive scans every stage computes its offsets with (tests / tools): out[i] = x[0] + ... + x[i-1], *total =
 * the sum of all n, where x[i] is in[i] (SHZ_SCAN_U32: u32 in, u32 out; SHZ_SCAN_U64: u64 in, u64 out) or
 * popcount(in[i]) (SHZ_SCAN_POPC64: u64 in, u32 out).  in / out / total are HOST arrays, out of n elements; total may be
 * NULL (the device scan then gets no total pointer).  in_place != 0 runs the device scan with its output on its input
 * (u32 and u64 only: SHZ_E_INVALID for popc64).  The 32-bit kinds form their sums in 32 bits: exact while the total is
 * at most 2^32 - 1.  n = 0: *total = 0. */
#define SHZ_SCAN_U32 0u
#define SHZ_SCAN_POPC64 1u
#define SHZ_SCAN_U64 2u
int32_t shz_scan_host(shz_ctx* ctx, uint32_t kind, const void* in, void* out, uint64_t n, uint32_t in_place,
                      uint64_t* total);

/* Query preparation (bench / tests): exact sum of squares of each clip (device PCM, clip-major, equal
 * lengths) to HOST, and out = clip(rint(sig + scale[c] * noise)) on the device: the digital form of
 * get_noise_from_sound + sf.write (recognizer_test.py:426-435, 557); twin: oracle/synth.mix_query. */
int32_t shz_sumsq_i16(shz_ctx* ctx, const int16_t* dev_pcm, uint32_t n_clips, uint64_t n_samples, uint64_t* out_host);
int32_t shz_mix_i16(shz_ctx* ctx, const int16_t* dev_sig, const int16_t* dev_noise, uint32_t n_clips,
                    uint64_t n_samples, const double* scale_host, int16_t* dev_out);

/* Pinned host memory for PCM (and any other array handed to the library): the reference's callers hold their samples in
 * host arrays (read(), __init__.py:70-113; recognizer.py:357-382); a decoder that writes them into a buffer from here lets
 * shz_fingerprint_batch feed the GPU by DMA at the link rate, chunk by chunk beside the kernels of the chunk before. */
int32_t shz_host_alloc(shz_ctx* ctx, uint64_t bytes, void** out);
int32_t shz_host_free(shz_ctx* ctx, void* p);   /* ctx may be NULL */

/* ---- extraction --------------------------------------------------------------------- */
/* Frames mlab produces for n_samples (mlab.specgram via __init__.py:232-237). */
uint32_t shz_frame_count(uint64_t n_samples);

/* Stage parity/debug: dB spectrogram of a batch, replaces
 *   mlab.specgram(x, NFFT=4096, Fs, window_hanning, noverlap=2048)[0] + 10*log10
 *   (__init__.py:232-241).  clip_off: n_clips+1 sample offsets into pcm (host memory).
 * out_db (HOST): per clip a float64 [2049, F_c] freq-major block (the reference's layout),
 * blocks concatenated in clip order; cap_doubles = capacity of out_db in doubles.
 * The logarithm is the correctly rounded one (csrc/shz_log10.h).  With SHZ_STFT_POWER the block holds what
 * specgram returns (the PSD before the log, __init__.py:232-237) in the staged form peak picking reads:
 * exact zeros read as 1.0, the power whose dB value is the 0.0 the reference assigns them (:241).
 * The power is computed with the reference's arithmetic operation by operation (numpy 2.x: pocketfft's radix-8 passes on the
 * complex frame, its complex product on a host with FMA3, mlab's scaling: csrc/shz_extract.hip np_fft4096): every value is
 * the one specgram returns, bit for bit (tests/golden/psd_digests.json).  The same arithmetic decides every tie of the
 * batch path (shz_peaks / shz_fingerprint_batch). */
int32_t shz_stft_db(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                    uint32_t fs, uint32_t flags, double* out_db, uint64_t cap_doubles, uint64_t* count);

/* The rows the fast STFT kernel stages for fp32 peak picking (tests / tools): stft_psd_kernel launched as the extraction
 * driver launches it (same clip tables, same grid and frame map) on a batch of HOST pcm, its rows copied to HOST memory
 * without their padding: out = [frames][2049] of float (SHZ_STAGE_F32: the kernel of every extraction call) or of double
 * (SHZ_STAGE_F64: the same arithmetic with the last conversion left out, which nothing else launches), frame-major, frames
 * of all clips in clip order at the ctx's hop (shz_set_overlap).  A value is the power as specgram scales it, an exact
 * zero staged as 1.0 (fp32: also a power that rounds to 0.0f).  The staging buffer is filled with 0xFF bytes first: a cell
 * the kernel does not write reads as a NaN.  flags: SHZ_STAGE_PERSISTENT launches the persistent grid (each eighth of the
 * frames walked by an eighth of the workgroups) whatever the frame count; without it the call takes chunks of 32 frames
 * once there are more frames than the persistent grid has room for 32 each, as the single pipeline does.  *frames (may be
 * NULL) = rows written.  One pass: SHZ_E_CAPACITY if the staged rows, the copied rows and the PCM exceed the workspace
 * limit.  SHZ_E_INVALID before anything runs: NULL buffers with work to do, an unknown kind or flag bit, clip_off not
 * non-decreasing, out_cap_rows below the frame count (*frames is set), more than 2^20 frames.  n_clips = 0: *frames = 0. */
#define SHZ_STAGE_F32 0u
#define SHZ_STAGE_F64 1u
#define SHZ_STAGE_PERSISTENT 1u
int32_t shz_stft_stage_host(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, uint32_t fs,
                            uint32_t kind, uint32_t flags, void* out, uint64_t out_cap_rows, uint64_t* frames);

/* The log transform alone, on the HOST (no device, no ctx): out_db[i] = 10*log10(power[i]) where power != 0, else 0.0
 * (__init__.py:241), with the same correctly rounded logarithm the kernels use (csrc/shz_log10.h) -- the function
 * that decides ties in the peak test, exposed so that tests can pin it without a GPU. */
int32_t shz_db_values(const double* power, uint64_t n, double* out_db);

/* Constellation peaks of a batch: replaces get_2D_peaks(10*log10(specgram)) +
 * the stable time sort at generate_hashes (__init__.py:116-177, 194-195).
 * Outputs (host unless SHZ_OUT_DEVICE): peak_f/peak_t in (clip, time asc, freq asc)
 * order, peak_off[n_clips+1] CSR offsets. */
int32_t shz_peaks(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                  uint32_t fs, double amp_min, uint32_t flags,
                  uint16_t* peak_f, uint32_t* peak_t, uint64_t* peak_off, uint64_t cap, uint64_t* count);

/* get_2D_peaks(arr2D, amp_min) on a caller-supplied 2-D float64 array (__init__.py:116-177):
 * arr2d is HOST, C-contiguous [n_rows(freq), n_cols(time)]; outputs in np.where row-major
 * order (freq asc, time asc) like the reference's return value. */
int32_t shz_peaks_from_db(shz_ctx* ctx, const double* arr2d, uint32_t n_rows, uint32_t n_cols,
                          double amp_min, uint32_t* out_f, uint32_t* out_t, uint64_t cap, uint64_t* count);

/* generate_hashes(peaks, fan_value) in packed form (__init__.py:179-210): peaks must be in
 * (time asc, freq asc) order per clip (peak_off CSR, host).  key32 = f1<<20 | f2<<8 | dt. */
int32_t shz_pair_hash(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                      uint32_t n_clips, uint32_t fan_value,
                      uint32_t* key32, uint32_t* t1, uint64_t* hash_off, uint64_t cap, uint64_t* count);

/* fingerprint() for a batch of channels (__init__.py:212-245): PCM -> (key32, t1) in the
 * reference's generation order, hash_off[n_clips+1] CSR offsets (always HOST).
 * key32/t1 are host unless SHZ_OUT_DEVICE. */
int32_t shz_fingerprint_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                              uint32_t fs, double amp_min, uint32_t fan_value, uint32_t flags,
                              uint32_t* key32, uint32_t* t1, uint64_t* hash_off, uint64_t cap, uint64_t* count);

/* Host PCM of 192 MB or more (no SHZ_PCM_DEVICE) is fed in chunks of whole clips (16 MB, then ~64 MB): a helper thread uploads chunk
 * i + 1 on its own stream while the extraction pass of chunk i runs -- the call's rate is the link's.  Results are those of
 * one pass.  SHZ_UPLOAD_PIPELINE=0 in the environment turns it off.  Counters since the context was created: chunks and
 * bytes that went that way, seconds the upload thread spent copying, seconds the passes waited for a chunk. */
int32_t shz_upload_stats(shz_ctx* ctx, uint64_t* chunks, uint64_t* bytes, double* copy_s, double* wait_s);

/* The window of mlab.specgram as fingerprint() calls it (__init__.py:232-237): NFFT = wsize = 4096 is what the STFT kernel is
 * built for (its radix plan, LDS layout and the 2049-bin peak stage); `noverlap = int(wsize * wratio)` is free: every
 * extraction call of the context then cuts frames x[k hop : k hop + 4096], hop = 4096 - noverlap (mlab:307-308), and a clip
 * of n >= 4096 samples has (n - 4096) / hop + 1 frames (shz_frame_count_hop; shz_frame_count is the default hop 2048).
 * noverlap >= 4096: SHZ_E_INVALID (mlab raises ValueError, mlab:242).  Other wsize: not implemented -- the Python layer raises
 * NotImplementedError, there is no CPU fallback. */
int32_t shz_set_overlap(shz_ctx* ctx, uint32_t noverlap);
/* numpy's tables for a window of nfft samples, as the fp64 path uses them (no GPU needed; any argument may be NULL):
 * window[nfft] = np.hanning(nfft) (mlab.window_hanning), twiddles[2 nfft] = (re, im) of the values pocketfft's
 * sincos_2pibyn(nfft) holds (cos, +sin of 2 pi i / nfft: the forward passes conjugate), *sumsq = (window ** 2).sum() in
 * numpy's pairwise order.  For tests: tests/test_numpy_tables.py compares them with numpy's own bits on the host. */
int32_t shz_numpy_tables(uint32_t nfft, double* window, double* twiddles, double* sumsq);
/* The window of the fp64 path as the host's numpy forms it: window[4096] = np.hanning(4096), sumsq = (window ** 2).sum()
 * (mlab.window_hanning and the scaling of mlab._spectral_helper behind __init__.py:232-237).  The Python layer calls this for
 * every context it creates, so the window is numpy's by construction; without the call the libm form of shz_numpy_tables is
 * used (equal to numpy's on the hosts seen).  The fast kernel behind the fp32 staging multiplies with the same table. */
int32_t shz_set_numpy_window(shz_ctx* ctx, const double* window, double sumsq);
/* How the host's numpy multiplies complex numbers (`np.conj(result) * result` in mlab._spectral_helper): fused = 1 (default):
 * real part fma(re, re, im * im) -- numpy's SIMD product on x86-64 with FMA3, the hosts of the fixtures; fused = 0:
 * re * re + im * im.  The Python layer probes its numpy when it creates a context and says which. */
int32_t shz_set_numpy_product(shz_ctx* ctx, int32_t fused);
/* mlab.specgram(x, NFFT=nfft, Fs, window_hanning, noverlap)[0] -> 10*log10 where != 0 (__init__.py:232-241) for window sizes
 * OTHER than 4096: nfft a power of two in [64, 2048].  A generic kernel (one workgroup per frame, radix-2 in fp64) -- correct,
 * not fast; the reference and every caller of it use 4096.  pcm: host, one channel; out_db: host [nfft/2 + 1][n_frames]
 * (the reference's layout), cap_doubles its capacity; SHZ_STFT_POWER: the PSD instead of dB.  With shz_peaks_from_db and
 * shz_pair_hash this is fingerprint(wsize=nfft) as the reference composes it.  Other sizes: SHZ_E_UNSUPPORTED (8192 has no
 * packed key: key32 gives a frequency 12 bits; non-powers of two are not implemented). */
int32_t shz_stft_db_any(shz_ctx* ctx, const int16_t* pcm, uint64_t n_samples, uint32_t fs, uint32_t nfft, uint32_t noverlap,
                        uint32_t flags, double* out_db, uint64_t cap_doubles, uint64_t* n_frames);
uint32_t shz_frame_count_hop(uint64_t n_samples, uint32_t hop);

/* Staging precision of shz_peaks / shz_fingerprint_batch.  Default (0): the power spectrogram is staged in fp32 and
 * the cells fp32 cannot decide (shared window maxima, threshold within 1e-7) are re-derived in fp64; results are
 * those of the fp64 path bit for bit.  1: stage fp64 and decide everything in the peak kernel (twice the HBM traffic;
 * what a clip falls back to on stationary / plateau material, and always used for amp_min < 0). */
int32_t shz_set_stage_f64(shz_ctx* ctx, int32_t enabled);
/* Counters since ctx creation: cells left undecided by the fp32 pass, those that needed fp64 values, FFT frames
 * recomputed for them, whole passes repeated with fp64 staging, single clips re-run with fp64 staging (windows with more
 * tied cells than the verification kernel takes: only those clips are redone and spliced into the batch) and the frames
 * of those clips.  Any pointer may be NULL. */
int32_t shz_extract_stats(shz_ctx* ctx, uint64_t* undecided, uint64_t* decided_f64, uint64_t* frames_recomputed,
                          uint64_t* f64_passes, uint64_t* f64_clips, uint64_t* f64_clip_frames);

/* sha1(f"{f1}|{f2}|{dt}")[:10 bytes] per key (__init__.py:207-208; BINARY(10) at
 * mysql_database.py:48).  key32: host or device (SHZ_IN_DEVICE); out10: host [n][10]. */
int32_t shz_sha1_prefix(shz_ctx* ctx, const uint32_t* key32, uint64_t n, uint32_t flags, uint8_t* out10);

/* Inverse of the above for hashes that arrive as hex/BINARY(10) from outside (a MySQL dump, another
 * process): the preimage space is only 2049 x 2049 x 201 strings, so the GPU hashes all of it and
 * looks the digests up.  digests10: host [n][10]; key32_out: host [n], 0xFFFFFFFF where no preimage
 * exists.  Lets insert_hashes / SELECT_MULTIPLE (mysql_database.py:62-68, 82-86) take foreign hashes. */
int32_t shz_sha1_invert(shz_ctx* ctx, const uint8_t* digests10, uint64_t n, uint32_t* key32_out);

/* ---- fingerprint table (replaces the MySQL fingerprints table, mysql_database.py:46-68) - */
int32_t shz_table_create(shz_ctx* ctx, shz_table** out);
int32_t shz_table_destroy(shz_table* t);
/* INSERT IGNORE of rows (hash, song_id, offset) (mysql_database.py:62-68, 167-181);
 * rows are staged; duplicates on (song_id, offset, hash) are dropped at finalize. */
int32_t shz_table_insert(shz_table* t, const uint32_t* key32, const uint32_t* sid, const uint32_t* off,
                         uint64_t n, uint32_t flags);
/* same, one song per clip: song id of clip c = sid0 + c, rows from a CSR (key32, t1, hash_off) */
int32_t shz_table_insert_clips(shz_table* t, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off,
                               uint32_t n_clips, uint32_t sid0, uint32_t flags);
/* sort staged+existing rows by (key, sid, off), drop duplicates, build the bucket index */
int32_t shz_table_finalize(shz_table* t);
/* Bulk build (the insert loop of fingerprint_directory, __init__.py:378-386, at database scale):
 * shz_table_reserve announces how many rows the table will hold and how many arrive between two seals; ONE slab for
 * the segments' columns, the run arena, the staging columns and the sort scratch are then allocated once, on a helper
 * thread beside the first fingerprint batches, and the build performs no further device allocation.  Without it
 * everything still works, allocating as it goes.  flags: SHZ_RESERVE_WAIT (return when the memory is there),
 * SHZ_RESERVE_GATHER: the table HOLDS its sealed runs in the arena (sized for all rows_hint rows, this rank's and its
 * peers') until shz_table_finalize / shz_table_allgather merges all of them at once -- seal_run never cuts a segment on
 * the way, so every row can still travel, and the one merge cuts segments by KEY RANGE (a query hash is then looked up
 * in one segment, not in all).  The flag takes effect with rows_hint = 0 too (nothing is allocated ahead then).
 * shz_table_seal_run turns the staged rows into a sorted run (bounded scratch: one batch; a run holds at most 2^32 - 4096
 * rows, more staged rows become several runs) WITHOUT making them visible to queries.  Without SHZ_RESERVE_GATHER full
 * segments are cut as soon as enough rows wait (bounded arena).  shz_table_finalize merges what is left (k-way merge of the runs, 8 bytes
 * read + 12 written per row) and makes everything visible.  On a table whose active segment holds rows, or whose song
 * ids + offsets need more than 32 bits, seal_run is finalize -- on a table that holds its runs it is SHZ_E_UNSUPPORTED
 * instead and the rows stay staged (rows put into segments could not travel any more). */
int32_t shz_table_reserve(shz_table* t, uint64_t rows_hint, uint64_t batch_rows_hint, uint32_t flags);
int32_t shz_table_seal_run(shz_table* t);
/* rows one sealed run may hold (0 = the hard limit, at most 2^32 - 4096 rows, which larger values are clamped to); small
 * values make many runs of few rows (tests) */
int32_t shz_table_set_run_rows(shz_table* t, uint64_t rows);
/* A table is a list of sorted segments (each one radix sort, < 2^32 rows; one cut from sealed runs holds at most
 * min(rows, 2^32 - 4096)) that every probe visits; rows beyond `rows` per segment open a new one at finalize.  Default 2^31; smaller values only for tests.
 * UNIQUE(song_id, offset, hash) + INSERT IGNORE (mysql_database.py:54-55, 62-68) hold across segments: staged rows
 * that already sit in a frozen segment are dropped at finalize, duplicates inside the batch by the sort.  The value may
 * change between calls: an active segment that already holds more rows is frozen as it is by the next batch that does not fit. */
int32_t shz_table_set_segment_rows(shz_table* t, uint64_t rows);
/* ON DELETE CASCADE of fingerprints when songs are deleted (mysql_database.py:57-58; DELETE_UNFINGERPRINTED :132-134,
 * the reference's crash recovery at __init__.py:424): every row of the listed song ids leaves the table (all segments
 * and the staged rows), the order of the rest is kept.  sids: host array of any 32-bit ids, listed or not in the table
 * (scratch: 4 bytes per listed id, whatever its value).  Sealed runs become segments first.  A finalized table whose last
 * rows leave stays finalized: it answers, with nothing, without another shz_table_finalize. */
int32_t shz_table_delete_songs(shz_table* t, const uint32_t* sids, uint64_t n_sids, uint64_t* rows_deleted);
/* DROP TABLE fingerprints: no rows, no segments; allocations of the active segment are kept for the rows to come.  A
 * finalized table stays finalized (empty); one that never was still refuses queries (SHZ_E_STATE). */
int32_t shz_table_clear(shz_table* t);
int32_t shz_table_rows(shz_table* t, uint64_t* n_rows, uint64_t* n_staged);
/* number of sorted segments the finalized rows live in (every query hash is looked up in each of them) */
int32_t shz_table_segments(shz_table* t, uint32_t* n_segments);
/* sorted rows to host (dump / parity): arrays of cap rows */
int32_t shz_table_export(shz_table* t, uint32_t* key32, uint32_t* sid, uint32_t* off, uint64_t cap, uint64_t* count);
/* SELECT hash, song_id, offset WHERE hash IN (keys) (SELECT_MULTIPLE, mysql_database.py:82-86;
 * recognizer.py:252-259): rows of every listed key, grouped in the order the keys are given,
 * inside a key ordered by (song_id, offset).  keys: host; outputs: host arrays of cap rows. */
int32_t shz_table_lookup(shz_table* t, const uint32_t* keys, uint64_t n_keys,
                         uint32_t* key32, uint32_t* sid, uint32_t* off, uint64_t cap, uint64_t* count);
/* distinct (hash, offset) rows of one song = songs.total_hashes candidates (__init__.py:381) */
int32_t shz_table_song_rows(shz_table* t, uint32_t sid, uint64_t* n_rows);
/* SELECT hash, offset FROM fingerprints WHERE song_id IN (sids): the rows of the listed songs, gathered on the device (the
 * reference has no such statement; its schema, mysql_database.py:34-58, would answer it).  Song sids[i] owns the rows
 * [row_off[i], row_off[i + 1]) of key32 / off, in list order (the list need not be sorted); inside a song the rows are
 * ordered by (key32, offset) ascending -- UNIQUE(song_id, offset, hash): no two are equal, the result is one fixed
 * sequence.  Rows come from every frozen segment and the active one.  A listed id without rows -- one above the table's
 * largest included -- owns an empty range.  sids, row_off (n_sids + 1 entries): host.  key32 / off: host arrays of cap rows,
 * device arrays with SHZ_SONGS_DEVICE_OUT, or BOTH NULL: counts only -- row_off is filled, no row is copied (the batched
 * shz_table_song_rows).  The song-id column is the only one read in full (twice, 4 bytes a row); keys and offsets are read
 * where a row hits; scratch grows with the hits and the listed ids, not with the table's rows (4 bytes per 1,024 rows).
 * SHZ_E_STATE: staged or unsealed rows (as shz_table_song_rows).  SHZ_E_INVALID, before anything is launched: NULL table,
 * NULL row_off, exactly one of key32 / off NULL, a song id listed twice.  SHZ_E_CAPACITY: more than cap rows -- row_off is
 * filled all the same, row_off[n_sids] is the room the call needs.  SHZ_E_UNSUPPORTED: 2^32 rows or more in one call.
 * n_sids == 0: SHZ_OK, row_off[0] = 0. */
#define SHZ_SONGS_DEVICE_OUT 128u /* shz_table_song_hashes: key32 / off are device memory */
int32_t shz_table_song_hashes(shz_table* t, const uint32_t* sids, uint32_t n_sids, uint64_t* row_off, uint32_t* key32,
                              uint32_t* off, uint64_t cap, uint32_t flags);

/* ---- match + align (replaces return_matches/align_matches, recognizer.py:222-338) ------- */
/* Queries are CSR: query q owns (key32, q_off) pairs [query_off[q], query_off[q+1]); duplicate
 * (key, q_off) pairs inside a query are collapsed (set semantics, recognizer.py:378-382).
 * Outputs (host), per query up to topn results ranked like align_matches:
 *   out_sid/out_delta/out_aligned [n_queries*topn]  (sid, db_off - q_off of the winning bin, its count)
 *   out_dedup  [n_queries*topn]  dedup_hashes[sid] (DB rows matched, once per row, recognizer.py:261-264)
 *   out_nres   [n_queries]       results valid for q
 *   out_nhash  [n_queries]       len(set(hashes)) = queried_hashes (recognizer.py:389)
 *   out_npairs [n_queries]       len(matches)
 * Votes are packed as (query, song id, delta + bias, flag) with sb = bits(largest song id), dbits = bits(largest table
 * offset + largest query offset of the sub-batch), qb = bits(queries of the sub-batch - 1), at least 1 bit each.
 * SHZ_E_UNSUPPORTED, exactly when (n_queries > 0):
 *   - the table holds an offset >= 2^31 (shz_table_maxima; out_delta is int32_t -- the reference's INT UNSIGNED
 *     column allows up to 2^32 - 1), or a query offset is >= 2^20;
 *   - a query with hashes does not fit the 64-bit key alone: 1 + sb + bits(largest table offset + its largest query
 *     offset) + 1 > 64.  Queries that fit alone but not together are split into smaller sub-batches; results are exact.
 */
int32_t shz_match_batch(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                        const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                        uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                        uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs);
/* recognize() for a batch of queries in one call (recognizer.py:377-392: fingerprint every channel, union the hashes,
 * return_matches, align_matches): shz_fingerprint_batch and shz_match_batch joined on the device -- the hashes are written
 * to buffers the library owns and matched there, none crosses the bus.  Clips as for shz_fingerprint_batch (pcm host, or
 * device with SHZ_PCM_DEVICE); query q owns the adjacent clips (its channels) [query_clip0[q], query_clip0[q + 1]):
 * query_clip0 has n_queries + 1 entries, starts at 0, does not decrease and ends at n_clips, else SHZ_E_INVALID before
 * anything is launched (as for topn outside [1, 64] or a table that is not finalized: SHZ_E_STATE).  There is no capacity
 * to pass and no SHZ_E_CAPACITY: the buffers are sized from the frame counts (shz_recognize_estimate) and the extraction
 * is repeated once with the room it asked for.  flags: SHZ_PCM_DEVICE, SHZ_MATCH_FULL_SORT.  Outputs: the seven of
 * shz_match_batch, same shapes and meaning -- the same arrays as the two calls give.  A single small query keeps the
 * queued one-workgroup fold (shz_match_spec_stats): its bias is the largest frame count of the clips - 1, which bounds
 * every t1.  ms_extract / ms_match (may be NULL): hipEvent times of the two halves on the ctx stream. */
int32_t shz_recognize_batch(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                            const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min, uint32_t fan_value,
                            uint32_t topn, uint32_t flags, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                            uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                            float* ms_extract, float* ms_match);
/* No GPU, no ctx: the entries the first extraction pass of shz_recognize_batch has room for, for clips of `frames` frames
 * in all (an input with more hashes takes the repeated pass). */
uint64_t shz_recognize_estimate(uint64_t frames, uint32_t fan_value);
/* Test switches that force the vote tiles' rare paths (never set in production): SHZ_DEBUG_VT_TINY_HEAVY gives the list
 * of ranges handed from vt_stream to vt_fold room for ONE range; SHZ_DEBUG_VT_PROBE1 lets an LDS hash probe give up
 * after one round (what a full table would cause).  Either way the pass's flag word is set, and the sub-batch is voted
 * again through the full sort (align_matches' result is a function of the votes, recognizer.py:289-338: same arrays).
 * shz_match_vt_redo: how many sub-batches went that way since the context was created. */
#define SHZ_DEBUG_VT_TINY_HEAVY 1u
#define SHZ_DEBUG_VT_PROBE1 2u
/* Test switch of the table build: the most rows a sealed run or a segment cut from runs may hold drops from 2^32 - 4096
 * to 65,536 (run cut, shz_table_set_run_rows clamp, segment cut, the size check of an exchange round), so that tests reach
 * the cuts at the limit with few rows.  Set it before the table's first call; every rank of a gathered build alike. */
#define SHZ_DEBUG_RUN_LIMIT_SMALL 4u
/* Test switch of shz_scan_batch: a group of windows handed to the match holds at most 3 windows, so that tests reach the
 * group borders with tiny inputs (results do not depend on the grouping). */
#define SHZ_DEBUG_SCAN_SMALL_GROUPS 8u
/* Test switch of shz_recognize_speeds: a slice of queries handed to the warp and the match holds at most 2 queries, so that
 * tests reach the slice borders with tiny inputs (results do not depend on the slicing). */
#define SHZ_DEBUG_SPEED_SMALL_SLICES 16u
/* Test switch of shz_scan_speeds: a slice holds at most 1 recording x 2 rungs and a group of windows handed to the match at
 * most 3 windows, so that tests reach the slice, chunk and group borders with tiny inputs (results do not depend on them). */
#define SHZ_DEBUG_SCAN_SPEED_SMALL_SLICES 32u
/* Test switch of shz_match_songs_warps: a slice holds one song x at most 2 warps, so that tests reach the slice and chunk
 * borders with tiny inputs (results do not depend on the slicing); of shz_match_songs_warps_extents: a slice holds at most 2
 * jobs. */
#define SHZ_DEBUG_CATALOG_SMALL_SLICES 64u
/* Test switch of the vote: the tolerant route (shz_set_vote_tolerance) is taken at tolerance 0 too, where it computes what
 * the other routes compute, so that its kernels can be compared with theirs on the same inputs. */
#define SHZ_DEBUG_VOTE_TOLERANT_ROUTE 128u
/* Test switch of shz_match_extents / shz_match_songs_extents: a tile of the extent kernel holds 64 pairs instead of 2,048,
 * its LDS table 4 (element, segment) descriptors instead of 512, and a sub-batch 3 queries instead of 4,096, so that tests
 * reach every border with tiny inputs (results do not depend on any of them). */
#define SHZ_DEBUG_EXTENT_SMALL_TILES 256u
/* Test switch of shz_repeats_* and shz_shared_*: a slice holds one recording (one job), an expand tile 64 pairs instead of
 * 2,048 and a block of the flag, count and cell kernels 64 elements instead of 256, so that tests reach every border with
 * tiny inputs (results do not depend on any of them). */
#define SHZ_DEBUG_REPEAT_SMALL_SLICES 512u
/* Test switch of the vote floor (shz_set_vote_floor): a match sub-batch holds at most 3 queries and the histogram kernels'
 * LDS table 2 queries instead of 32, so that tests reach the sub-batch border, the table's border and the direct global
 * adds with tiny inputs (results do not depend on the switch). */
#define SHZ_DEBUG_FLOOR_SMALL 1024u
/* Test switch of the song filter (shz_set_song_filter): with a filter set, a block of the two filter kernels holds 64 votes
 * instead of 2,048 and a match sub-batch at most 3 queries, so that tests reach the block, wave and sub-batch borders with
 * tiny inputs (results do not depend on the switch). */
#define SHZ_DEBUG_FILTER_SMALL 2048u
int32_t shz_set_debug(shz_ctx* ctx, uint32_t flags);
/* The vote's tolerance, a setting of the context that holds for its later calls (default 0).  With c[sid][d] the votes of a
 * query per song and offset difference d = db_off - q_off, and S(sid, d) = the sum of c[sid][d .. d + bins]: a song's
 * `aligned` is the largest S over the windows that start at an occupied d (the first one in ascending d where several reach
 * it), its `delta` the bin inside that window with the largest count of its own (the smaller delta where bins tie); songs
 * rank by aligned descending, then song id ascending.  dedup, nres, nhash, npairs do not depend on it, and bins = 0 is the
 * plain vote of one bin (align_matches), bit for bit.  A window holds votes of its own (query, song) only.  Every call that
 * votes inside the library follows it: shz_match_batch, shz_match_device_host, shz_recognize_batch, shz_recognize_speeds /
 * _warps, shz_scan_batch / _speeds / _warps, shz_listeners_push*, shz_match_songs / _warps and shz_pairs_vote;
 * shz_match_pairs, whose votes leave as they are, does not.  With bins > 0 the votes go one way: 8-byte votes in one pass
 * over a sub-batch, the full sort, then a fold over runs of equal (query, song, delta) -- neither the vote tiles, the 4-byte
 * votes nor the fold queued ahead of the count (shz_match_spec_stats) are taken.  bins > 31: SHZ_E_INVALID, the setting
 * stays as it was.  A NULL ctx (or NULL bins): SHZ_E_INVALID. */
int32_t shz_set_vote_tolerance(shz_ctx* ctx, uint32_t bins);
int32_t shz_get_vote_tolerance(shz_ctx* ctx, uint32_t* bins);
/* The vote floor, a setting of the context that holds for its later calls (default off): how far chance reaches for a query.
 * With c(s, d) the votes of a query per song s and offset difference d, and a count c >= 1 put into one of 32 buckets --
 * c - 1 for c <= 16 (buckets 0 .. 15 are the exact counts 1 .. 16), else min(31, floor(log2 c) + 12) (bucket 16: 17 .. 31,
 * bucket 17: 32 .. 63, ..., bucket 31: everything from 2^19 up; shz_vote_bucket) -- every query handed to a vote records one
 * ROW of two exact histograms, 32 + 32 uint32_t:
 *   bin_hist[b]   the bins (s, d) with c(s, d) >= 1 whose count falls into bucket b -- single bins, whatever the tolerance;
 *   song_hist[b]  the songs with any vote whose best count falls into bucket b: the value the vote reports as `aligned` for
 *                 that song (the largest c(s, d); under shz_set_vote_tolerance the best window sum).
 * A query without hashes or without a match records two zero rows.  sum(song_hist) = the songs with a vote; with topn at
 * least that, the bucketed `aligned` column is song_hist; where every bin count is <= 16, sum((b + 1) bin_hist[b]) = npairs.
 * While it is on, the votes go one way, as under a tolerance: 8-byte votes in one pass over a sub-batch, the full sort, the
 * fold over runs at the tolerance in force, and two histogram kernels over the runs and the fold's records; the rows come
 * back with the result block (no extra round trip).  Every result array is what it is with the setting off.  Rows are kept
 * in host memory owned by the context, in the order the queries were handed to the vote (every call listed at
 * shz_set_vote_tolerance; a caller that skips the vote because nothing is to be looked up records zero rows, so the rows of
 * a call line up with its result arrays; shz_match_pairs records nothing, shz_pairs_vote records the rows of its votes; a
 * refused call records nothing).  A ROW COSTS 256 BYTES OF HOST MEMORY UNTIL IT IS TAKEN: take them call by call.
 * shz_set_vote_floor(on = 0) drops the rows not yet taken.  shz_vote_floor_rows: the rows recorded since the last take.
 * shz_vote_floor_take copies them, in order, into song_hist / bin_hist ([cap][32] each) and clears the store, *n = their
 * number; with more rows than cap it returns SHZ_E_CAPACITY with *n = the number needed, copies nothing and clears nothing.
 * shz_vote_bucket: the bucket of a count (no GPU, no ctx; count 0 or a NULL bucket: SHZ_E_INVALID). */
int32_t shz_set_vote_floor(shz_ctx* ctx, uint32_t on);
int32_t shz_get_vote_floor(shz_ctx* ctx, uint32_t* on);
int32_t shz_vote_floor_rows(shz_ctx* ctx, uint64_t* n);
int32_t shz_vote_floor_take(shz_ctx* ctx, uint32_t* song_hist, uint32_t* bin_hist, uint64_t cap, uint64_t* n);
int32_t shz_vote_bucket(uint32_t count, uint32_t* bucket);
/* The song filter, a setting of the context that holds for its later calls (default: none): match within a set of songs.  A
 * FILTERED MATCH ON A TABLE GIVES THE ARRAYS THAT THE PLAIN MATCH GIVES ON A TABLE HOLDING ONLY THE ALLOWED SONGS' ROWS.
 * n_sets sets of song ids as a CSR: set s owns sids[set_off[s] .. set_off[s + 1]); ids in any order, repeats allowed; an
 * empty set is legal (it allows nothing; with SHZ_FILTER_EXCLUDE it denies nothing).  n_sets = 0 clears the filter (sids,
 * set_off and flags are not looked at).  Query q keeps the votes of song s iff bit(set(q), s) != exclude, where
 * bit(set, s) = s is listed in the set and exclude = flags & SHZ_FILTER_EXCLUDE.  set(q) is set_of_query[q] in
 * shz_match_batch_sets (and shz_match_device_host_sets) and set 0 EVERYWHERE ELSE: shz_match_batch, shz_match_device_host
 * and every call that matches inside the library (shz_recognize_batch, shz_recognize_speeds / _warps, shz_scan_batch /
 * _speeds / _warps, shz_listeners_push*, shz_match_songs / _warps), whose queries are windows, variants and listed songs the
 * caller never sees.  While a filter is set: out_npairs counts the KEPT pairs; out_nhash is the query's alone, as ever;
 * out_dedup keeps its meaning (a row belongs to one song); with the vote floor on, both histograms are those of the kept
 * votes; shz_match_stats keeps counting the probed pairs.  shz_match_pairs and shz_pairs_vote (the sharded match) return
 * SHZ_E_UNSUPPORTED while a filter is set: nothing ignores it silently.  With no filter set nothing changes.
 * The library builds one bitmap per set on the host, words = largest listed id / 32 + 1 for all sets (a song id beyond the
 * bitmap counts as not listed), and keeps them in a device block the context owns until the filter is cleared, replaced or
 * the context destroyed; the filter belongs to no table.  The votes then go one way, as under a tolerance: 8-byte votes in
 * one pass over a sub-batch; between the expand and the sort a stable compaction drops the barred votes (a count kernel, a
 * scan of the block counts, a write kernel) and the kept total is read back -- one more small round trip a vote pass; then
 * the full sort and the fold over runs at the tolerance in force.
 * Refused, the previous setting staying in force: a NULL ctx, a NULL set_off, a NULL sids with ids listed, set_off[0] != 0,
 * a set_off that decreases, flag bits other than SHZ_FILTER_EXCLUDE (SHZ_E_INVALID); bitmaps of more than 2^31 bytes
 * together (SHZ_E_UNSUPPORTED); no memory for them (SHZ_E_NOMEM).
 * shz_get_song_filter: the sets, the flags and the ids listed over all sets as given (each pointer may be NULL).
 * shz_match_batch_sets: shz_match_batch with the set of every query; SHZ_E_STATE with no filter set, SHZ_E_INVALID for a
 * NULL set_of_query or an entry >= n_sets, both before anything is launched. */
#define SHZ_FILTER_EXCLUDE 1u
int32_t shz_set_song_filter(shz_ctx* ctx, const uint32_t* sids, const uint64_t* set_off, uint32_t n_sets, uint32_t flags);
int32_t shz_get_song_filter(shz_ctx* ctx, uint32_t* n_sets, uint32_t* flags, uint64_t* n_ids);
int32_t shz_match_batch_sets(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                             const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                             uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                             uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs, const uint32_t* set_of_query);
/* The key cap, a setting of the context that holds for its later calls (default 0: off): keys that hold too many table rows
 * vote for nobody.  WITH CAP c >= 1 A MATCH GIVES THE ARRAYS THAT THE PLAIN MATCH GIVES ON A TABLE LACKING EVERY ROW WHOSE KEY
 * HOLDS MORE THAN c ROWS.  The rows of a key are counted over all segments together (the distinct (key, song, offset) rows
 * that shz_table_export shows); a key with exactly c rows stays.  The cap is a property of table and cap, not of the query:
 * a key is dropped for every query or for none.  out_sid / delta / aligned / dedup / nres / npairs and the vote floor's
 * histograms describe the kept votes; out_nhash is the query's alone, as ever.  It is decided at the probe: one kernel
 * between the probe and the scan of its counts zeroes the counts of the dropped (query, key) groups, so the expand, the
 * sort and the fold never see their votes, on every route, and no host round trip is added.  shz_match_stats: pairs are
 * those expanded (after the cap), rows_scanned stay as probed.  Every call that matches inside the library follows it (the
 * list at shz_set_vote_tolerance), and so do shz_match_pairs -- a key lives on one shard, so the sharded match applies the
 * cap exactly -- and shz_match_extents / _fit, whose counts, frames, histograms and moments then cover kept pairs only.
 * With the cap off every call launches the kernels it launched before.  Changing the cap forgets the context's estimate of
 * votes per hash that sizes the next sub-batch.
 * shz_key_cap_stats: the (query, key) groups and the pairs dropped by the last match call, over all its sub-batches (both
 * 0 with the cap off; each pointer may be NULL).
 * shz_table_key_hist: the key sizes of a table's finalized rows (SHZ_E_STATE with staged rows): keys[b] = the distinct keys
 * whose row count falls into bucket b of shz_vote_bucket (1 .. 16 exact, then powers of two), rows[b] = the rows they hold,
 * *max_rows = the largest key, *n_keys = the distinct keys (both may be NULL).  An empty table gives zeros.  One kernel per
 * segment over its sorted key column; a key that several segments hold is counted once, with the rows of all. */
int32_t shz_set_key_cap(shz_ctx* ctx, uint64_t rows);
int32_t shz_get_key_cap(shz_ctx* ctx, uint64_t* rows);
int32_t shz_key_cap_stats(shz_ctx* ctx, uint64_t* groups_dropped, uint64_t* pairs_dropped);
int32_t shz_table_key_hist(shz_table* t, uint64_t keys[32], uint64_t rows[32], uint64_t* max_rows, uint64_t* n_keys);
int32_t shz_match_vt_redo(shz_ctx* ctx, uint64_t* count);
/* A single query of at most 8,192 hashes handed over in host memory has its vote kernels queued before the number of its
 * votes is known (they do nothing when it exceeds 32,768; the call then continues as for any other query): how many
 * calls queued them / took their results from them, since the context was created.  Same results either way;
 * SHZ_MATCH_NO_SPEC=1 in the environment turns the queueing off. */
int32_t shz_match_spec_stats(shz_ctx* ctx, uint64_t* queued, uint64_t* used);
/* The match as shz_recognize_batch, shz_recognize_speeds, shz_scan_batch, shz_scan_speeds and shz_listeners_push run it
 * (tests / tools): on query columns that already lie on the device, with the bound of the query offsets those callers know
 * without reading them.  key32 / q_off / query_off are HOST arrays as for shz_match_batch; the two columns are copied into
 * device buffers the call allocates and frees, and the library's internal match on device columns runs on them unchanged.
 * Outputs and refusals as shz_match_batch (flags: SHZ_MATCH_FULL_SORT only).  bias_bound: a promise that every q_off is
 * <= bias_bound; below 0 or >= 2^32: no bound.  With a bound, ONE query of at most 8,192 hashes has its vote kernels queued
 * ahead of the count (shz_match_spec_stats) on the layout the BOUND gives -- dbits = bits(largest table offset + bias_bound)
 * -- where that layout fits the one-workgroup fold: 1 + sb + dbits <= 32, dbits <= 20, topn <= 8, bias_bound < 2^20, no
 * SHZ_MATCH_FULL_SORT (and the table's last match does not promise this one more than 65,536 votes: hashes x its votes per
 * hash).  Their results are the answer when the votes number at most 32,768 and no offset exceeded the bound;
 * otherwise (and for a bound that does not hold) they are dropped and the call goes through the vote passes on the layout
 * of the offsets themselves.  The same arrays for every bound. */
int32_t shz_match_device_host(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                              const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags, int64_t bias_bound,
                              uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                              uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs);
/* ... with the set of every query under a song filter, as shz_match_batch_sets takes and refuses it (tests / tools). */
int32_t shz_match_device_host_sets(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                   const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                                   int64_t bias_bound, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                   uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                                   const uint32_t* set_of_query);
/* Which of the table's own songs are the same recording: every listed song matched against the REST of the table in one
 * call, without its audio.  shz_table_song_hashes gathers the songs' rows on the device (song sids[q] is query q, its
 * offsets are the query offsets), the library's match on device columns runs on them with topn + 1 and the table's largest
 * offset as the bound of the query offsets, and the song itself is taken out of its own list on the host.  That is exact:
 * rows are unique per (hash, song, offset), so for one delta a query row pairs with at most one row of any song -- no song's
 * aligned count exceeds the query's row count, which the song itself reaches at delta 0.  Among the topn + 1 results it is
 * dropped and the exact top topn of the others remain; where it is missing (more than topn other songs tie with it and carry
 * smaller ids) the first topn are that list already.  Outputs (host): the seven arrays of shz_match_batch for "every other
 * song", same shapes and meaning ([n_sids * topn] / [n_sids], zero past out_nres), and out_rows[n_sids] (may be NULL), the
 * songs' row counts.  out_nhash equals out_rows (a song's rows are distinct).  out_npairs is what the match counts: the
 * song's pairs with its own rows are included.  out_dedup of a result is the rows of that song under the listed song's
 * hashes, as for any query.
 * topn in [1, 63] and flags SHZ_MATCH_FULL_SORT only, a song id listed twice: SHZ_E_INVALID.  The match's refusals pass
 * through (SHZ_E_STATE for a table that is not finalized; offsets >= 2^31 in the table); a listed song holding an offset
 * >= 2^20 is SHZ_E_UNSUPPORTED -- it is a query offset here -- and 2^32 gathered rows or more in one call likewise (list
 * fewer songs a call).  One table on one GPU: a key-sharded table has no call like it. */
int32_t shz_match_songs(shz_ctx* ctx, shz_table* t, const uint32_t* sids, uint32_t n_sids, uint32_t topn, uint32_t flags,
                        uint64_t* out_rows, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                        uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs);
/* ---- match extents (new): WHERE in the query and in the song the aligned hashes lie.  A match answers (song, delta,
 * aligned); delta says how the two timelines are shifted, not over which stretch the match holds.  This is a second pass
 * over the same (query hash, table row) pairs for candidates the caller names -- usually the winners of a match.
 * Definitions (tests/extent_twin.py is the same in Python): the table's rows (key, sid, off) and a query's hashes (key, q_off)
 * are sets (duplicate hashes of a query collapse, as in the match); a PAIR is a (hash, row) of equal key with d = off - q_off
 * (signed); it BELONGS to candidate (sid, d_lo, d_hi) when row.sid == sid and d_lo <= d <= d_hi, and to every candidate whose
 * test it passes -- two candidates of a query may name one song with disjoint or overlapping ranges.  shift of a query = the
 * smallest s >= 0 with (its largest q_off >> s) < 64, 0 for an empty query.  Per candidate: out_count = pairs that belong;
 * out_q_first / out_q_last = the smallest / largest q_off among them; out_t_first / out_t_last = the smallest / largest off;
 * out_hist[64] (may be NULL: not computed) = pairs that belong per bucket q_off >> shift.  All of them are 0 where count is 0.
 * sum(hist) == count, and with d_lo == d_hi == the delta of a result of shz_match_batch at tolerance 0, count == its aligned.
 * All arrays are HOST arrays: key32 / q_off / query_off as for shz_match_batch; the candidates [n_queries * ncand], slot c of
 * query q at q * ncand + c, of which query q uses the first cand_n[q]; the outputs [n_queries * ncand] ([... * 64] for
 * out_hist, [n_queries] for out_shift), zero at and past cand_n[q].  The outputs are written only by a call that returns
 * SHZ_OK.  The vote tolerance of the context does not enter: the ranges are explicit.  Integer adds, minima and maxima only:
 * exact and repeatable.
 * Refused, before anything is launched: a NULL ctx, table or required array, ncand outside [1, 64], a cand_n[q] > ncand, a
 * used candidate with d_lo > d_hi, a query_off that decreases (SHZ_E_INVALID); a table with staged or unsealed rows, or not
 * finalized (SHZ_E_STATE, as the match); a query offset >= 2^20 or a table offset >= 2^31 (SHZ_E_UNSUPPORTED, as the match).
 * n_queries == 0: SHZ_OK, nothing is written. */
int32_t shz_match_extents(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off, const uint64_t* query_off,
                          uint32_t n_queries, uint32_t ncand, const uint32_t* cand_sid, const int32_t* cand_dlo,
                          const int32_t* cand_dhi, const uint32_t* cand_n, uint32_t* out_count, uint32_t* out_q_first,
                          uint32_t* out_q_last, uint32_t* out_t_first, uint32_t* out_t_last, uint32_t* out_hist,
                          uint32_t* out_shift);
/* shz_match_extents with the MOMENTS of every candidate's pairs (new; tests/fit_twin.py is the same in Python): the arguments
 * and the contract above, and four more outputs, HOST arrays of [n_queries * ncand], all required.  For candidate (sid, d_lo,
 * d_hi) and every pair that belongs to it let q = q_off and u = d - d_lo, so 0 <= u <= d_hi - d_lo:
 *     out_sum_q = sum q    out_sum_u = sum u    out_sum_qq = sum q^2    out_sum_qu = sum q u      (unsigned 64 bits, modulo 2^64)
 * all 0 where count is 0 and at and past cand_n[q].  They are what a least-squares line d = slope q + intercept through the
 * pairs needs (shazam_amd/extent.py: line_fit): a query that runs at another tempo than the rung it was warped with lets d
 * drift along q, and the slope says by how much.  Integer adds only: exact and repeatable.  The seven other outputs equal
 * shz_match_extents' on the same inputs.  A used candidate with d_hi - d_lo >= 4096 is refused (SHZ_E_UNSUPPORTED, before
 * anything is launched): below that q u < 2^32, so sum_q, sum_u and sum_qu cannot wrap, and sum_qq wraps only from 2^24 pairs
 * on.  A NULL sum array: SHZ_E_INVALID. */
int32_t shz_match_extents_fit(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off, const uint64_t* query_off,
                              uint32_t n_queries, uint32_t ncand, const uint32_t* cand_sid, const int32_t* cand_dlo,
                              const int32_t* cand_dhi, const uint32_t* cand_n, uint32_t* out_count, uint32_t* out_q_first,
                              uint32_t* out_q_last, uint32_t* out_t_first, uint32_t* out_t_last, uint32_t* out_hist,
                              uint32_t* out_shift, uint64_t* out_sum_q, uint64_t* out_sum_u, uint64_t* out_sum_qq,
                              uint64_t* out_sum_qu);
/* The catalogue form: the listed songs' rows are gathered on the device as shz_match_songs gathers them and are the queries
 * (song sids[q] is query q, its offsets are the query offsets; no row crosses the bus).  Candidates and outputs as above with
 * n_sids in place of n_queries.  A candidate may be the listed song itself: at d_lo = d_hi = 0 its count is the song's row
 * count.  Refused as above, and: a song id listed twice (SHZ_E_INVALID, before anything is launched); 2^32 gathered rows or
 * more in one call, a listed song holding an offset >= 2^20 -- it is a query offset here -- (SHZ_E_UNSUPPORTED; the latter is
 * seen on the device, after the gather).  n_sids == 0: SHZ_OK. */
int32_t shz_match_songs_extents(shz_ctx* ctx, shz_table* t, const uint32_t* sids, uint32_t n_sids, uint32_t ncand,
                                const uint32_t* cand_sid, const int32_t* cand_dlo, const int32_t* cand_dhi, const uint32_t* cand_n,
                                uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first,
                                uint32_t* out_t_last, uint32_t* out_hist, uint32_t* out_shift);
/* ---- sped-up and pitch-shifted copies inside the table (new): shz_match_songs finds a re-upload only while its audio is
 * bit-identical; a copy pitched up 3 %, a 25/24 video transfer or a rip from a drifting deck shares no hash with its
 * original.  The table holds no peaks, so the peak-level warp of shz_warp_pair_hash_tf cannot be applied to a stored song --
 * but a row (key32 = f1 << 20 | f2 << 8 | dt, offset = t1) IS the two peaks (f1, t1) and (f2, t1 + dt).  The ROW WARP moves
 * both with the maps of shz_warp_pair_hash_tf and forms the key again.  For a row (key32, off) and a warp (t16, f16), each
 * factor Q16 in [32768, 131072], in 64-bit integers:
 *     f1, f2, dt = key32 >> 20, (key32 >> 8) & 0xFFF, key32 & 0xFF
 *     t1' = (off t16 + 32768) >> 16            t2' = ((off + dt) t16 + 32768) >> 16          dt' = t2' - t1'
 *     f1' = (2 65536 f1 + f16) / (2 f16)       f2' likewise
 *     kept iff f1' <= 2048 and f2' <= 2048 and dt' <= 200;   out = (f1' << 20 | f2' << 8 | dt',  t1')
 * Elementwise: no sort, no fan_value, nothing is deduplicated (two rows may meet in one (key, t1'); the match collapses them
 * and its out_nhash counts the distinct ones).  At (65536, 65536) the output is the input.  t1' is stored in 32 bits: offsets
 * < 2^31, the table's own limit for matching, keep it exact at every factor.  Relation to the peak-level warp: for t16 >=
 * 65536 and f16 >= 65536 the row warp of a song's hashes equals shz_warp_pair_hash_tf of its peaks entry for entry (the
 * order of the peaks is the input's, no peak leaves, dt' >= dt keeps every pair's rank); below unity the peak-level warp
 * pairs again after frames merge and peaks leave, and a few per cent of the entries differ.  Numpy twin:
 * tests/rows_warp_twin.py.
 *
 * shz_warp_row_host (no GPU, no ctx): the map over n rows on the host -- the one inline function the kernels call.
 * out_keep[i] = 1 where row i is kept; out_key32[i] / out_off[i] hold its image there and 0 elsewhere (nothing is compacted).
 * SHZ_E_INVALID: a factor outside the range, a NULL array with n > 0.
 *
 * shz_warp_rows: the rows of n_songs songs -- song q owns [row_off[q], row_off[q + 1]), row_off: HOST, n_songs + 1 entries;
 * key32 / off host, or device with SHZ_IN_DEVICE -- at every warp v = (tempo_q16[v], pitch_q16[v]).  OUTPUT ORDER: for song
 * q, for warp v, the kept rows of q in their input order -- (q, v) is one contiguous query of the match.  out_row_off (HOST,
 * n_songs n_warps + 1 entries in (q, v) order, may be NULL) is the CSR of those segments, exact: the rows are counted before
 * they are written.  out_key32 / out_off: host, or device with SHZ_OUT_DEVICE; more than cap kept rows: SHZ_E_CAPACITY,
 * *count = required, out_row_off written, nothing else (the two-call idiom of shz_warp_pair_hash).  The places come from a
 * scan of block counts: no atomic decides where a row lands, and the output is repeatable.  SHZ_E_INVALID before anything is
 * launched: n_warps of 0 or above 1024, a NULL table, a factor of either table outside the range, a row_off that decreases.
 * SHZ_E_UNSUPPORTED: rows x n_warps of 2^32 or more in one call. */
int32_t shz_warp_row_host(const uint32_t* key32, const uint32_t* off, uint64_t n, uint32_t t16, uint32_t f16,
                          uint32_t* out_key32, uint32_t* out_off, uint8_t* out_keep);
int32_t shz_warp_rows(shz_ctx* ctx, const uint32_t* key32, const uint32_t* off, const uint64_t* row_off, uint32_t n_songs,
                      const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags,
                      uint32_t* out_key32, uint32_t* out_off, uint64_t* out_row_off, uint64_t cap, uint64_t* count);
/* shz_match_songs at a list of warps: the listed songs' rows are gathered as shz_match_songs gathers them (into columns the
 * call owns), warped at every warp by the row warp above, and every (song q, warp v) is one query of the library's match on
 * device columns, with topn + 1 and the bias bound (largest listed offset x largest t16 + 32768) >> 16; the song itself is
 * taken out of each of its lists on the host -- dropping one element from the top topn + 1 leaves the exact top topn of the
 * others at any warp.  Outputs (host), ALL variants, (q, v) at index q n_warps + v: out_sid / out_delta / out_aligned /
 * out_dedup [n_sids n_warps topn], out_nres / out_nhash / out_npairs [n_sids n_warps] (the last two may be NULL), zero past
 * out_nres; out_rows[n_sids] (may be NULL), the songs' unwarped row counts.  There is no best-of fold: an exact copy found at
 * the identity must not hide a pitched copy of the same song found at another warp.  out_delta is the found song's frame
 * under the listed song's WARPED frame 0.  out_nhash is the number of distinct warped rows of (q, v).  With the single warp
 * (65536, 65536) the arrays equal shz_match_songs's.
 * Refused: everything shz_match_songs refuses; n_warps of 0 or above 1024, a NULL table, a factor outside the range
 * (SHZ_E_INVALID, before anything is launched); a listed offset whose image under the largest t16 reaches 2^20
 * (SHZ_E_UNSUPPORTED; the message names the offset and the factor).
 * SLICES: the work goes in slices of (whole songs x a contiguous chunk of warps) whose items -- rows x warps, 8 bytes each in
 * the call's warped columns -- stay below 2^32, within 1/8 of the workspace limit and the match's 2^28-pair budget; the ladder
 * is cut only where one song at all warps is beyond that.  The call's buffers are allocated once, for the largest slice.
 * Results do not depend on the slicing (SHZ_DEBUG_CATALOG_SMALL_SLICES).  ms_gather / ms_warp / ms_match (may be NULL):
 * hipEvent times of the gather, of the warp stages (with their one read-back a slice) and of the matches. */
int32_t shz_match_songs_warps(shz_ctx* ctx, shz_table* t, const uint32_t* sids, uint32_t n_sids, uint32_t topn,
                              const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags,
                              uint64_t* out_rows, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                              uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                              float* ms_gather, float* ms_warp, float* ms_match);
/* WHERE an altered copy overlaps its original, and at what tempo (new): the extent pass of shz_match_extents_fit on songs of
 * the table warped by the row warp, one JOB a query.  Job j is (job_sid[j], job_t16[j], job_f16[j]) -- usually a pair
 * shz_match_songs_warps found, at the warp it was found at; one song may stand in several jobs at different warps.  The
 * query of job j is the set { row warp of (key32, off) under (job_t16[j], job_f16[j]), kept } over the rows of song
 * job_sid[j]; the outputs are exactly those of shz_match_extents_fit on those queries and the given candidates (candidates
 * and outputs [n_jobs * ncand], [n_jobs * ncand * 64] for out_hist, which may be NULL, [n_jobs] for out_shift; the four sums
 * are required).  out_q_first / out_q_last are WARPED frames of the listed song (shazam_amd/extent.py: own_frames takes them
 * back to its own), out_t_first / out_t_last frames of the candidate song.  out_kept[n_jobs] (may be NULL): the kept warped
 * rows of every job BEFORE the set collapses rows that meet in one (key, t1'); out_count counts the set.  A song without
 * rows, or a job whose rows all leave under its warp, is an empty query: its outputs are zero.  With every job at (65536,
 * 65536) on distinct songs the seven extent arrays equal shz_match_songs_extents' and the sums shz_match_extents_fit's on
 * the songs' gathered rows.  Numpy twin: tests/rows_fit_twin.py.
 * Every distinct song is gathered ONCE, on the device, as shz_match_songs gathers it (no row crosses the bus); the JOB FORM
 * of the row warp lays the work out over (job, row of its song) items, job-major, counts the kept rows per block and per
 * job, scans, and writes job after job, the kept rows of a job in input order: a job is one contiguous query and the CSR
 * over the jobs is exact (no atomic decides where a row lands).
 * Refused before anything is launched: what shz_match_songs_extents and shz_match_extents_fit refuse (the table's state, ncand
 * outside [1, 64], a cand_n above ncand, d_lo > d_hi, a NULL array: SHZ_E_INVALID / SHZ_E_STATE; a used candidate of 4,096
 * bins or more, a table offset >= 2^31: SHZ_E_UNSUPPORTED); a factor outside [32768, 131072], a NULL job array with n_jobs
 * > 0 (SHZ_E_INVALID).  Refused after the gather: a listed offset whose image under its job's t16 reaches 2^20 -- it is a
 * query offset here -- (SHZ_E_UNSUPPORTED; the message names the offset and the factor); 2^32 gathered rows or more, or 2^32
 * items (rows over all jobs) or more in one call (SHZ_E_UNSUPPORTED).  n_jobs == 0: SHZ_OK, nothing is written.  The outputs
 * are written only by a call that returns SHZ_OK.
 * SLICES: the jobs go in slices of whole jobs whose items -- 8 bytes each in the call's warped columns -- stay within 1/8 of
 * the workspace limit, each slice through the extent pass (which cuts its queries into sub-batches of its own); the call's
 * buffers are allocated once, for the largest slice.  Under SHZ_DEBUG_CATALOG_SMALL_SLICES a slice holds at most 2 jobs;
 * SHZ_DEBUG_EXTENT_SMALL_TILES acts as in shz_match_extents.  Results do not depend on the slicing.  ms_gather / ms_warp /
 * ms_extent (may be NULL): hipEvent times of the gather, of the warp stages (with their one read-back a slice) and of the
 * extent passes. */
int32_t shz_match_songs_warps_extents(shz_ctx* ctx, shz_table* t, const uint32_t* job_sid, const uint32_t* job_t16,
                                      const uint32_t* job_f16, uint32_t n_jobs, uint32_t ncand, const uint32_t* cand_sid,
                                      const int32_t* cand_dlo, const int32_t* cand_dhi, const uint32_t* cand_n,
                                      uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first,
                                      uint32_t* out_t_last, uint32_t* out_hist, uint32_t* out_shift, uint64_t* out_sum_q,
                                      uint64_t* out_sum_u, uint64_t* out_sum_qq, uint64_t* out_sum_qu, uint64_t* out_kept,
                                      float* ms_gather, float* ms_warp, float* ms_extent);
/* rows streamed / pairs voted by the last shz_match_batch (for HBM accounting) */
int32_t shz_match_stats(shz_ctx* ctx, uint64_t* rows_scanned, uint64_t* pairs, uint64_t* distinct_keys);

/* ---- multi-GPU database build (new) ---------------------------------------- */
/* RCCL communicator, one rank per GPU.  id: 128-byte ncclUniqueId made by rank 0 and shipped
 * to the other ranks by the host (a file, a socket, any key-value store the launcher offers). */
int32_t shz_comm_unique_id(uint8_t id_out[128]);
int32_t shz_comm_create(shz_ctx* ctx, const uint8_t id[128], int32_t rank, int32_t nranks, shz_comm** out);
/* The same communicator interface with the ranks as THREADS of one process (one context each, on one device or on several):
 * exchanges are rendezvous + device copies out of the peers' buffers.  Lets the N > 1 logic of the sharded build run on a
 * one-GPU box (tests), and a single process drive several GPUs without RCCL.  group_id: any number the ranks agree on. */
int32_t shz_comm_create_local(shz_ctx* ctx, uint64_t group_id, int32_t rank, int32_t nranks, shz_comm** out);
int32_t shz_comm_destroy(shz_comm* c);
/* The gathered build (the reference's analogue is the pool + insert loop of fingerprint_directory,
 * __init__.py:341, 357-386, which overlaps fingerprinting of the next song with the insert of the last).
 * Collective calls: every rank of the communicator makes them, on tables reserved with SHZ_RESERVE_GATHER.
 *
 * shz_table_exchange_run: the staged rows become a sorted run (as shz_table_seal_run) and ONE exchange round runs: all
 *   ranks all-gather a 320-byte block (largest song id / offset so far, flags, row counts and song-id ranges of the runs
 *   they have sealed and not yet sent -- up to 16 a round, each < 2^32 rows), agree on one packing layout from the global
 *   maxima, and every rank's announced runs start travelling to every peer, 8 bytes a row in pieces of <= 1 GB, each
 *   pair of GPUs on its own xGMI link (grouped ncclSend / ncclRecv), on the communicator's own stream: the call returns
 *   with the transfers in flight, and the next batch is fingerprinted beside them.  Ranks need not call it equally often.
 * shz_table_allgather: seals what is staged, runs rounds until every rank has arrived here and sent all its runs, waits
 *   for the transfers, and merges ALL runs -- its own and its peers' -- in one k-way merge into segments cut by key range
 *   (more than 32 runs: the smallest are merged first).  No rank sorts another rank's rows.  Afterwards every rank
 *   holds the same table.  Which rows travel: everything inserted since the table was last finalized / gathered --
 *   staged rows and sealed runs.
 * The column path: when any rank's table already holds rows, or its song ids + offsets need more than 32 bits, the
 *   ranks' STAGED rows travel as unsorted columns and finalize sorts them into the table each rank holds.  Every rank
 *   takes it if any rank needs it.  Sealed runs do not travel on it: if any rank holds one, or its seal_run has already
 *   moved rows into segments (a table not reserved with SHZ_RESERVE_GATHER that sealed past a segment's worth), EVERY
 *   rank returns SHZ_E_STATE -- never a table that differs between ranks.
 * bytes_recv: payload bytes this rank received (all rounds of this build). */
int32_t shz_table_exchange_run(shz_table* t, shz_comm* c);
int32_t shz_table_allgather(shz_table* t, shz_comm* c, uint64_t* bytes_recv);
/* exchange rounds / payload bytes received / host seconds spent waiting for peers and transfers since the last
 * shz_table_allgather, and the runs the arena holds now.  Any pointer may be NULL. */
int32_t shz_table_exchange_stats(shz_table* t, uint64_t* rounds, uint64_t* bytes_recv, double* wait_s, uint32_t* runs_held);
/* The sort + merge + segments half of the above without a communicator: the staged rows are n_runs consecutive
 * blocks of run_rows[r] rows (what n_runs ranks would have staged); the result equals shz_table_finalize's. */
int32_t shz_table_finalize_runs(shz_table* t, const uint64_t* run_rows, uint32_t n_runs);
/* seconds the last shz_table_allgather / shz_table_finalize_runs spent sorting its own rows, inside exchange rounds
 * (host time: waiting for peers and for transfers, queueing them -- with pipelined rounds most of a transfer runs beside
 * fingerprinting and shows up nowhere), merging the runs and cutting segments.  Any pointer may be NULL. */
int32_t shz_table_build_stats(shz_table* t, double* sort_s, double* exchange_s, double* merge_s, double* segments_s);
/* Host seconds the table spent per phase of the build since the last reset (stream drained at each phase border):
 * staging allocation, insert, INSERT-IGNORE anti-join against frozen segments, segment top-up, maxima, sort, merge,
 * unique + scan, column allocation, compaction into columns, bucket index, slicing, release of the staging columns.
 * The reference's analogue is the per-file wall time of fingerprint_directory's insert loop (__init__.py:378-386).
 * seconds: host array of cap entries (may be NULL); *n = number of phases; shz_table_phase_name(i) names phase i. */
int32_t shz_table_phase_stats(shz_table* t, double* seconds, uint32_t cap, uint32_t* n, int32_t reset);
const char* shz_table_phase_name(uint32_t i);
int32_t shz_comm_barrier(shz_comm* c);
/* Collective: one tiny exchange of each kind the gathered build uses, on the communicator's exchange stream.  RCCL connects
 * two ranks when they first talk to each other; a build whose time matters calls this before its clock starts. */
int32_t shz_comm_warmup(shz_comm* c);

/* ---- key-sharded table (new; SURVEY.md 8f row 4: the table no longer fits one GPU) -------
 * Rows are partitioned by a hash of key32, so a DB row lives on exactly one shard and both quantities
 * align_matches needs are sums over shards: dedup_hashes[sid] (recognizer.py:261-264) and the
 * (sid, offset difference) histogram (recognizer.py:305).  Build: every rank stages its own tracks' rows,
 * shz_table_shard_exchange routes each row to the rank that owns its key (all-to-all over RCCL) and
 * finalizes.  Query: every rank runs shz_match_pairs on the same queries, shz_pairs_allgather collects the
 * packed votes, shz_pairs_vote ranks them: the same kernels as shz_match_batch on the unsharded table. */
/* shard (0..nshards-1) of each key; host arrays */
int32_t shz_shard_of_keys(const uint32_t* key32, uint64_t n, uint32_t nshards, uint32_t* shard_out);
/* drop the STAGED rows that do not belong to `shard` (several shards on one GPU, tests) */
int32_t shz_table_keep_shard(shz_table* t, uint32_t shard, uint32_t nshards);
/* append the STAGED rows of src that belong to `shard` to dst's staged rows (src unchanged), and forget a
 * table's staged rows: one staging table feeding several shard tables on one GPU */
int32_t shz_table_stage_from(shz_table* dst, shz_table* src, uint32_t shard, uint32_t nshards);
int32_t shz_table_clear_staged(shz_table* t);
/* route every rank's STAGED rows to the owner of their key, then finalize; bytes_recv: payload received */
int32_t shz_table_shard_exchange(shz_table* t, shz_comm* c, uint64_t* bytes_recv);
/* Votes travel packed, 8 bytes each, in ONE layout all shards agree on:
 *   ((query << sid_bits | song_id) << delta_bits | (db_off - q_off) + bias) << 1 | counts-a-DB-row-once flag
 * sid_bits >= bits of the largest song id of the WHOLE table, bias >= the largest q_off of the batch,
 * delta_bits >= bits of (largest offset of the whole table + bias); bits(n_queries-1) + sid_bits + delta_bits + 1
 * must fit 64, and delta_bits <= 32 (tables hold offsets < 2^31, as for shz_match_batch); else SHZ_E_UNSUPPORTED.  shz_table_maxima gives a table's largest song id / offset (after shz_table_shard_exchange:
 * of the whole sharded table). */
int32_t shz_table_maxima(shz_table* t, uint32_t* max_sid, uint32_t* max_off);
/* probe + expand only (the head of shz_match_batch): the votes of this table's rows for the queries, appended
 * to a DEVICE buffer of cap entries.  More than cap: SHZ_E_CAPACITY with *count = the number needed.
 * The table holds shard `shard` of `nshards` (1 shard: everything): only the query hashes that shard owns are
 * looked up, so S shards together do the work of one table.
 * out_nhash / out_npairs (host, may be NULL): per query the distinct hashes / matches found HERE -- both add up
 * over shards, because every hash and every DB row belongs to exactly one of them. */
int32_t shz_match_pairs(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                        const uint64_t* query_off, uint32_t n_queries, uint32_t flags,
                        uint32_t shard, uint32_t nshards, uint32_t sid_bits, uint32_t delta_bits, uint32_t bias,
                        uint64_t* d_pairs, uint64_t cap, uint64_t* count, uint32_t* out_nhash, uint64_t* out_npairs);
/* all-gather the ranks' votes (device in, device buffer of cap entries out) */
int32_t shz_pairs_allgather(shz_comm* c, uint64_t n_local, const uint64_t* d_pairs, uint64_t* d_all, uint64_t cap,
                            uint64_t* n_total);
/* the tail of shz_match_batch over any collection of votes in that layout: sort, per (query, song) fold, top-n
 * ranked like align_matches (recognizer.py:289-338).  d_pairs (device, 16-byte aligned) is overwritten.  n < 2^32.
 * Outputs (host) as in shz_match_batch. */
int32_t shz_pairs_vote(shz_ctx* ctx, uint64_t* d_pairs, uint64_t n, uint32_t n_queries, uint32_t sid_bits,
                       uint32_t delta_bits, uint32_t bias, uint32_t topn, uint32_t* out_sid, int32_t* out_delta,
                       uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres);

/* ---- live streams (new; the reference's recogniser reads its input CHUNK = 8192 samples at a time per channel,
 * recognizer.py:21-25, 357-392) --------------------------------------------------------------------------------------
 * n_streams independent streams on one ctx.  The hashes a stream has emitted, concatenated over all its pushes, are
 * those of shz_fingerprint_batch on its whole signal, bit for bit and in order.  A frame t is SETTLED once frame t + 10
 * exists (its 21x21 peak window is complete; at the stream's end every frame is); a push extracts, per stream, one window
 * clip from frame max(0, settled - 10) to its last complete frame and keeps the peaks of the newly settled frames.  A
 * settled peak emits all its hashes once fan_value - 1 settled peaks follow it, or once the settled horizon H exceeds its
 * frame + 200, or when the stream ends; the rest (at most fan_value - 1 peaks) waits for the next push.
 * hop = the ctx's hop (shz_set_overlap) at creation; if it changes afterwards, calls return SHZ_E_STATE.
 * fan_value in [1, 64]; n_streams in [1, 65535].  Not thread-safe, like the ctx. */
typedef struct shz_streams shz_streams;
int32_t shz_streams_create(shz_ctx* ctx, uint32_t n_streams, uint32_t fs, double amp_min, uint32_t fan_value,
                           shz_streams** out);
int32_t shz_streams_destroy(shz_streams* s);
/* Append pcm[chunk_off[i] .. chunk_off[i+1]) to stream i (empty chunks allowed; chunk_off must not decrease); streams whose
 * bit is set in `end` (n_streams bits, may be NULL) end after this chunk -- a stream of fewer than 4096 samples emits the
 * hashes of its one zero-padded frame.  Outputs: the hashes that became final in this push, (key32, t1) with t1 in
 * absolute frames of the stream, stream i's at [hash_off[i], hash_off[i+1]) (hash_off: n_streams + 1, HOST).
 * SHZ_PCM_DEVICE / SHZ_OUT_DEVICE as for shz_fingerprint_batch.  SHZ_E_CAPACITY: *count = required and NO stream has
 * changed (repeat the call with room).  A stream that has ended: SHZ_E_STATE if it gets samples or an end bit, left alone
 * otherwise. */
int32_t shz_streams_push(shz_streams* s, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                         uint32_t flags, uint32_t* key32, uint32_t* t1, uint64_t* hash_off, uint64_t cap, uint64_t* count);
/* start stream slots afresh (ended or not): sample 0, nothing pending */
int32_t shz_streams_reset(shz_streams* s, const uint32_t* which, uint32_t n);
/* stream i: samples received, settled frames H, peaks pending, hashes emitted so far (any pointer may be NULL) */
int32_t shz_streams_state(shz_streams* s, uint32_t i, uint64_t* samples, uint64_t* settled, uint64_t* pending,
                          uint64_t* emitted);
/* No GPU, no ctx (like shz_frame_count_hop): the window plan of one push of a stream that had samples_before samples and
 * settled_before settled frames and has samples_after now (ending: it ends with them).  win_frame0 = first frame of the
 * window clip, [win_s0, win_s1) its samples, settled_after = the new horizon H (settled_after == settled_before: nothing
 * settles, no window; a stream that ends with 0 samples has one window of 0 samples, its one zero-padded frame).  SHZ_E_INVALID for hop outside [1, 4096], samples_after < samples_before or a settled_before that is not a
 * horizon of the stream. */
int32_t shz_stream_plan(uint64_t samples_before, uint64_t samples_after, uint64_t settled_before, uint32_t hop,
                        int32_t ending, uint64_t* win_frame0, uint64_t* win_s0, uint64_t* win_s1, uint64_t* settled_after);


/* ---- device-resident listeners (new; the loop around recognize() that reads a microphone, recognizer.py:357-392, for many
 * listeners at once) ---------------------------------------------------------------------------------------------------
 * n_listeners listeners over the streams of `s`: listener l is the `channels` = n_streams / n_listeners adjacent streams
 * [l channels, (l + 1) channels) (n_listeners must divide the streams: else SHZ_E_INVALID), whose hashes are unioned
 * (recognizer.py:377-382).  Each listener keeps, ON THE DEVICE, the window of its settled hashes (key32, absolute t1) with
 * t1 >= w0 = max(0, H - window_frames), H the smallest settled horizon of its channels (shz_listener_window).  The object
 * does not own the streams or the table; both must outlive it and belong to one ctx.  While it exists, push and reset the
 * streams through it only.  Not thread-safe, like the ctx. */
typedef struct shz_listeners shz_listeners;
int32_t shz_listeners_create(shz_streams* s, shz_table* t, uint32_t n_listeners, uint32_t window_frames, shz_listeners** out);
int32_t shz_listeners_destroy(shz_listeners* L);
/* One shz_streams_push (pcm, chunk_off, end: per STREAM, as there; device output into buffers of the object, repeated with
 * room on its SHZ_E_CAPACITY), the new hashes merged into the windows and the expired ones dropped on the device, and ALL
 * listeners recognised in one match on the device-resident windows with query offsets t1 - w0: what `offset` means for a
 * clip recorded from frame w0.  Outputs as shz_match_batch with n_queries = n_listeners (a listener whose window is empty:
 * nres = nhash = 0; an ended listener keeps its window and is matched again), plus out_w0[n_listeners] (may be NULL).
 * flags: SHZ_PCM_DEVICE, SHZ_MATCH_FULL_SORT.  Bad arguments, topn outside [1, 64], a table that is not finalized, a hop
 * that changed since the streams were created (SHZ_E_STATE) and whatever shz_streams_push refuses leave every stream and
 * every window as they were. */
int32_t shz_listeners_push(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end, uint32_t topn,
                           uint32_t flags, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                           uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs, uint32_t* out_w0);
/* start LISTENERS afresh: their streams (shz_streams_reset) and their windows */
int32_t shz_listeners_reset(shz_listeners* L, const uint32_t* which, uint32_t n);
/* listener l: hashes in its window, and the w0 of its last push (any pointer may be NULL) */
int32_t shz_listeners_state(shz_listeners* L, uint32_t l, uint64_t* window_hashes, uint64_t* w0);
/* The content of listener l's window (tests / tools): its entries in the order the device keeps them -- what the last push
 * kept of the old window, then what it kept of the new hashes -- copied to the HOST arrays key32 / t1 (absolute frames) /
 * q_off (t1 - w0 as the last push handed it to the match) of cap entries each; *n = their number (the window_hashes of
 * shz_listeners_state).  More than cap: SHZ_E_CAPACITY with *n = the number needed, nothing copied.  The call waits for
 * the ctx stream and changes no state.  q_off is meaningful only after a push: a listener that was reset has no entries,
 * and before the first push there is nothing to read. */
int32_t shz_listeners_window(shz_listeners* L, uint32_t l, uint32_t* key32, uint32_t* t1, uint32_t* q_off, uint64_t cap,
                             uint64_t* n);
/* ---- listeners at a ladder: peak windows (new; a station that plays its songs a few percent fast is a live feed) ----------
 * A warp acts on PEAKS (shz_warp_pair_hash_tf), so a window of hashes cannot be warped.  shz_listeners_create_peaks takes the
 * arguments of shz_listeners_create and refuses what it refuses; the object it makes keeps, on the device and per channel, the
 * settled peaks (f, t) of the channel's stream with t >= w0, in the stream's order (t ascending, f ascending).  w0 = max(0, H -
 * window_frames), H the smallest settled horizon of the listener's channels (shz_listener_window).  No cut is made at H: a
 * channel that runs ahead keeps its settled peaks.  The streams are exact, so channel c's window is the peaks of shz_peaks on
 * the stream's whole signal with w0 <= t < H_c (after its end: every peak with t >= w0).
 * The two kinds do not mix: shz_listeners_push and shz_listeners_window on a peak-window object, and shz_listeners_push_warps /
 * _push_speeds / _peaks / _timing on a hash-window object, are SHZ_E_STATE and change nothing.  reset, destroy and state work
 * on both; on a peak-window object shz_listeners_state reports as window_hashes the out_nhash of the last push's chosen
 * variant (0 before any push and after a reset). */
int32_t shz_listeners_create_peaks(shz_streams* s, shz_table* t, uint32_t n_listeners, uint32_t window_frames, shz_listeners** out);
/* One shz_streams_push (pcm, chunk_off, end: per STREAM, as for shz_listeners_push), the newly settled peaks appended to the
 * windows and the expired ones dropped on the device, then listener l at warp v = (tempo_q16[v], pitch_q16[v]) as one query:
 * exactly the hashes shz_warp_pair_hash_tf yields for a query whose clips are l's channels, their peak lists the windows
 * rebased to t - w0, at the streams' fan_value; query offsets are the warped t1'.  All n_listeners x n_warps queries go
 * through the match, in slices of whole listeners cut as shz_recognize_warps cuts its queries (SHZ_DEBUG_SPEED_SMALL_SLICES:
 * two listeners a slice); results do not depend on the slicing.  Outputs per listener as shz_recognize_warps' per query:
 * out_best[n_listeners] the variant with the greatest rank-0 aligned count (ties: the smallest |t16 - 65536| + |f16 - 65536|,
 * then the lower index), that variant's rows in out_sid / out_delta / out_aligned / out_dedup [n_listeners topn], out_nres,
 * out_nhash (may be NULL), out_profile [n_listeners n_warps] (may be NULL), out_w0[n_listeners] (may be NULL).  out_delta is in
 * the TABLE's frames: the song frame that lies at stream frame w0.  A listener without peaks in its window: nres = nhash = 0.
 * An ended listener keeps its window and is matched again at this push's ladder: the ladder belongs to the push, not to the
 * object, and a caller may narrow it once a station's speed is known.
 * Refused before the streams are pushed, every stream and every window staying as it was: what shz_listeners_push refuses;
 * n_warps of 0 or above 1024, a NULL table, a factor outside [32768, 131072] (SHZ_E_INVALID); flags other than SHZ_PCM_DEVICE |
 * SHZ_MATCH_FULL_SORT; a largest warped time round((max_c H_c - w0 - 1) max tempo / 65536) >= 2^20 over the listeners, the
 * query offsets of the match (SHZ_E_UNSUPPORTED; the horizons after the push follow from shz_stream_plan).
 * NOT a bit-for-bit twin of shz_listeners_push at a ladder of {65536}: the hash windows hold the hashes the streams have
 * emitted -- pending peaks have not paired yet, and a hash with t1 >= w0 stays whatever its partner -- while the peak
 * windows pair the window's peaks among themselves.  The exact equivalence is with shz_warp_pair_hash_tf on the window's peaks
 * (shz_listeners_peaks). */
int32_t shz_listeners_push_warps(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                                 uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps,
                                 uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                 uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile,
                                 uint32_t* out_w0);
/* shz_listeners_push_warps with the one table speed_q16 for time and frequency: a speed ladder (as shz_recognize_speeds is to
 * shz_recognize_warps; what is refused about the ladder names n_speeds / speed) */
int32_t shz_listeners_push_speeds(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                                  uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds, uint32_t flags, uint32_t* out_best,
                                  uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                                  uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, uint32_t* out_w0);
/* The window of channel `channel` of listener l (tests / tools): its peaks in the device's order, f and ABSOLUTE t, copied to
 * the HOST arrays of cap entries each; *n = their number.  More than cap: SHZ_E_CAPACITY with *n = the number needed, nothing
 * copied.  The call waits for the ctx stream and changes no state. */
int32_t shz_listeners_peaks(shz_listeners* L, uint32_t l, uint32_t channel, uint16_t* f, uint32_t* t, uint64_t cap, uint64_t* n);
/* Tools: ms (4 floats, may be NULL) = the hipEvent times of the last timed shz_listeners_push_warps -- the streams' push, the
 * window kernels with their read-back, the warp, the match -- and pushes from now on are timed (enable != 0) or not.  Timing
 * adds event waits to a push; it is off at creation. */
int32_t shz_listeners_timing(shz_listeners* L, int32_t enable, float* ms);
/* No GPU, no ctx (like shz_stream_plan): the window of a listener whose channels have settled[0 .. channels) frames:
 * *horizon = their minimum H, *w0 = max(0, H - window_frames). */
int32_t shz_listener_window(const uint64_t* settled, uint32_t channels, uint32_t window_frames, uint64_t* horizon, uint64_t* w0);

/* ---- resampling (new; the reference hands a file's frame_rate through and fixes the microphone at 44.1 kHz,
 * __init__.py:70-113, recognizer.py:21-27, so audio at another rate never meets the table) ---------------------------
 * Rational resampling fs_in -> fs_out of a batch of clips by an integer polyphase filter: g = gcd(fs_in, fs_out),
 * L = fs_out / g, M = fs_in / g, taps[L][T] int32 in Q30 (HOST, row p = phase p).  With x the clip (zero outside it),
 * p = (m M) mod L and i0 = (m M) div L + T / 2:
 *     out[m] = sat16((sum_{k < T} taps[p][k] * x[i0 - k] + 2^29) >> 30)      (arithmetic shift, sum exact in 64 bits)
 * clips as for shz_fingerprint_batch (pcm host, or device with SHZ_PCM_DEVICE; clip_off: n_clips + 1 sample offsets, HOST);
 * clips never read each other's samples.  Per clip and optional (NULL: 0, and every output m in [0, ceil(n L / M))):
 * in_base[c] = absolute index of the clip buffer's first sample -- x[i] is buffer[i - in_base] inside the buffer and 0
 * elsewhere -- and the outputs wanted, m in [m_first[c], m_end[c]) (both or neither): a chunk of a stream with the tail of
 * the chunk before in front of it gives the samples the whole stream gives.  out: int16 (host, or device with
 * SHZ_OUT_DEVICE), clip c's at [out_off[c], out_off[c + 1]) (out_off: HOST); cap in samples, SHZ_E_CAPACITY with *count =
 * required.  SHZ_E_INVALID before anything is launched: L, M or T of 0, odd T, T > SHZ_RESAMPLE_MAX_TAPS, a clip_off that
 * decreases, m_end < m_first.  SHZ_E_UNSUPPORTED: L or M above SHZ_RESAMPLE_MAX_RATIO, L * T above SHZ_RESAMPLE_MAX_TABLE.
 * shz_get_kernel_ms(which = 5) accumulates the kernel's time. */
#define SHZ_RESAMPLE_MAX_TAPS 4096u
#define SHZ_RESAMPLE_MAX_RATIO (1u << 24)
#define SHZ_RESAMPLE_MAX_TABLE (1u << 24)
int32_t shz_resample_i16(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, uint32_t L, uint32_t M,
                         uint32_t T, const int32_t* taps, const uint64_t* in_base, const uint64_t* m_first, const uint64_t* m_end,
                         uint32_t flags, int16_t* out, uint64_t* out_off, uint64_t cap, uint64_t* count);

/* ---- scanning long recordings (new; the monitoring loop around recognize(), recognizer.py:357-392 -- record a stretch,
 * fingerprint every channel, union the hashes, match, align -- for every overlapping stretch of a recording at once) -----
 * "Which songs play in this recording, and when?"  Every recording is fingerprinted ONCE; its device-resident hash list is
 * cut into overlapping time windows and all windows are matched together (hashes come out in generation order,
 * recognizer.py:100-114: t1 never decreases inside a clip, so a window is a contiguous range of each channel's list).
 * Recording r owns the adjacent clips (its channels) [rec_clip0[r], rec_clip0[r + 1]), as query_clip0 of
 * shz_recognize_batch; F_r = the largest shz_frame_count_hop of its channels at the ctx's hop.  It has W_r =
 * shz_scan_window_count(F_r, ...) windows: 0 without clips, 1 if F_r <= window_frames, else
 * ceil((F_r - window_frames) / step_frames) + 1.  Window w starts at frame s = w step_frames; its query is the set, over all
 * channels of the recording, of (key32, t1 - s) for the hashes with s <= t1 < s + window_frames, and the result of the scan
 * is shz_match_batch on exactly those queries: the seven arrays, windows recording-major, win_off[n_recs + 1] their CSR
 * (written whenever the arguments are valid, also with SHZ_E_CAPACITY).
 * EDGES: a window's hashes are a SUBSET of the whole recording's hashes.  They are not what fingerprinting the cut audio
 * would give: a peak near a cut is judged against its neighbours beyond the cut, a pair whose anchor lies in the window
 * counts although its partner lies behind the window's end, and one whose anchor lies in front of it does not.
 * window_frames >= F_r: the one window is the whole recording and the arrays are shz_recognize_batch's.
 * Refused before anything is launched: rec_clip0 / clip_off that are not as for shz_recognize_batch, window_frames of 0 or
 * >= 2^20 (the query offsets of the match), step_frames of 0, topn outside [1, 64] (SHZ_E_INVALID), a table that is not
 * finalized (SHZ_E_STATE), cap_windows (the room of the outputs, in windows) below the total: SHZ_E_CAPACITY with *count =
 * the total, which follows from the frame counts alone.  flags: SHZ_PCM_DEVICE, SHZ_MATCH_FULL_SORT.  Windows go to the
 * match in groups whose replicated columns fit 1/8 of the workspace limit (shz_set_workspace_limit); a group never splits a
 * window and the results do not depend on the grouping (SHZ_DEBUG_SCAN_SMALL_GROUPS).  A recording is extracted in one
 * pass: one of more than 2^20 frames is refused as shz_fingerprint_batch refuses it.  ms_extract / ms_window / ms_match
 * (may be NULL): hipEvent times of the extraction, of cutting the windows (bounds, scan, read-back, gathers) and of the
 * matches.  out_nhash / out_npairs may be NULL. */
uint64_t shz_scan_window_count(uint64_t frames, uint32_t window_frames, uint32_t step_frames);   /* no GPU, no ctx; frames 0: 0 */
int32_t shz_scan_batch(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                       const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                       uint32_t window_frames, uint32_t step_frames, uint32_t topn, uint32_t flags, uint64_t* win_off,
                       uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres,
                       uint32_t* out_nhash, uint64_t* out_npairs, uint64_t cap_windows, uint64_t* count, float* ms_extract,
                       float* ms_window, float* ms_match);
/* The timeline of a scan (no GPU, no ctx): the rank-0 answers folded into segments.  Inputs: win_off and out_sid / out_delta /
 * out_aligned (stride topn, rank 0 is read) / out_nres of shz_scan_batch.  Window w of a recording (w counts from the
 * recording's first window) is a HIT iff nres >= 1 and its rank-0 aligned >= min_aligned; its identity is (sid, shift),
 * shift = delta - w step_frames in 64 bits: song frame minus recording frame, constant while one song plays.  The windows
 * of a recording are visited in order with one open segment: a hit with the open segment's identity and
 * w - w_last - 1 <= max_gap extends it; any other hit closes it and opens a new one; a window without a hit changes
 * nothing; the recording's end closes it.  Per segment (recording-major, in order): recording, sid, shift, first and last
 * window, hit windows, largest aligned count.  Two-call idiom: more than cap segments: SHZ_E_CAPACITY, *count = their
 * number, the first cap are written (cap = 0: the seg_* pointers may be NULL). */
int32_t shz_scan_timeline(const uint64_t* win_off, uint32_t n_recs, const uint32_t* out_sid, const int32_t* out_delta,
                          const uint32_t* out_aligned, const uint32_t* out_nres, uint32_t topn, uint32_t step_frames,
                          uint32_t min_aligned, uint32_t max_gap, uint32_t* seg_rec, uint32_t* seg_sid, int64_t* seg_shift,
                          uint32_t* seg_first, uint32_t* seg_last, uint32_t* seg_hits, uint32_t* seg_best, uint64_t cap,
                          uint64_t* count);
/* ---- scan extents (new): frame-accurate start and end of every segment.  A segment's span is only as fine as the windows:
 * it starts at the start of its first hit window and ends at the end of its last one, and the music may begin or end
 * anywhere inside them.  The scan holds every recording's hashes on the device and knows each segment's identity (sid,
 * shift), so the extent pass of shz_match_extents can say where the aligned pairs of a segment really lie.
 * ZONES (shz_scan_zones; no GPU, no ctx; tests/scan_extent_twin.py is the same in Python): with a = first and b = last window
 * of a segment, W = window_frames, S = step_frames, M = margin_frames and F = frames[rec], every segment gets three half-open
 * ranges [lo, hi) of recording frames, zone z of segment i at 3 i + z:
 *   0 whole  [max(0, aS - M), min(F, bS + W + M))   all pairs of the play, its span in the song, a coarse histogram
 *   1 head   [max(0, aS - M), min(F, aS + W))       where the play starts: 64 buckets over W + M frames whatever its length
 *   2 tail   [bS,             min(F, bS + W + M))   where the play ends, likewise
 * An interrupted song gives two segments of one identity (rec, sid, shift), whose margins must not reach into each other's
 * windows: with L = the largest b_k S + W over EARLIER segments of the same identity, the lo of zones 0 and 1 is at least
 * min(L, aS); with R = the smallest a_k S over LATER ones, the hi of zones 0 and 2 is at most max(R, bS + W).  Every bound is
 * then clamped into [0, F]; a zone with lo >= hi after that (a window that starts behind the recording's end when S > W) is
 * EMPTY and is written as hi = lo.  Positions are formed in 64 bits.
 * Refused (SHZ_E_INVALID): window_frames or step_frames of 0, a NULL array (frames with n_recs > 0, the others with n_segs >
 * 0), a frames[r] >= 2^32, a segment with first > last or rec >= n_recs, segments that are not in the order shz_scan_timeline
 * emits (recordings ascending, inside a recording first > the last of the segment in front). */
int32_t shz_scan_zones(const uint32_t* seg_rec, const uint32_t* seg_sid, const int64_t* seg_shift, const uint32_t* seg_first,
                       const uint32_t* seg_last, uint64_t n_segs, const uint64_t* frames, uint32_t n_recs, uint32_t window_frames,
                       uint32_t step_frames, uint32_t margin_frames, uint32_t* zone_lo, uint32_t* zone_hi);
/* Everything in one call: the extraction (once), the window stage and the match of shz_scan_batch, shz_scan_timeline on the
 * host inside the library (min_aligned, max_gap), the zones, and the extent pass on the zones' hashes, which are cut from the
 * device-resident hash lists and never cross the bus.  The arguments up to `count` and ms_extract / ms_window / ms_match are
 * shz_scan_batch's, and the window arrays and win_off are array for array what it writes; seg_* [cap_segs] and *seg_count
 * are what shz_scan_timeline writes from them.
 * The QUERY of a zone is the set, over the recording's channels, of (key32, t1 - lo) for the hashes with lo <= t1 < hi -- the
 * cut of a window (EDGES above apply); its one CANDIDATE is (sid, shift + lo - d_tol, shift + lo + d_tol), because
 * off - (t1 - lo) = (off - t1) + lo and off - t1 is the shift; its RESULT is what shz_match_extents defines for that query
 * and candidate.  Zone outputs, [3 cap_segs] each, zone z of segment i at 3 i + z: zone_lo / zone_hi (the zone itself),
 * zone_count, zone_q_first / zone_q_last (in RECORDING frames, + lo, where count > 0; 0 otherwise), zone_t_first /
 * zone_t_last (song frames), zone_shift (of the zone's histogram: the smallest s with ((largest t1 - lo) >> s) < 64) and
 * zone_hist [3 cap_segs x 64] (bucket (t1 - lo) >> shift; may be NULL: not computed).  With d_tol = 0 and the context's
 * vote tolerance 0, zone 0's count of a one-window segment at margin 0 is that window's rank-0 aligned count, and zone 0's
 * count of any segment is at least the segment's seg_best (every window's hash set is a subset of zone 0's).  ms_extent (may
 * be NULL): hipEvent time of cutting the zones and of the extent pass.
 * More segments than cap_segs: SHZ_E_CAPACITY, *seg_count = their number, the window arrays and the first cap_segs segments
 * are written and NO zone output is: zone outputs only ever come from a call that returns SHZ_OK.  There are never more
 * segments than windows.  No segment (or no window): SHZ_OK, *seg_count = 0, nothing is launched for zones.
 * Refused before anything is launched, in this order behind shz_scan_batch's own refusals: d_tol > 31, margin_frames >= 2^20,
 * a NULL seg_count or, with cap_segs > 0, a NULL segment or zone array (SHZ_E_INVALID); then the table as shz_match_extents
 * refuses it (a table offset >= 2^31: SHZ_E_UNSUPPORTED).  Seen on the device, after the scan: a zone longer than 2^20 frames
 * (a query offset of the extent pass; SHZ_E_UNSUPPORTED) -- a play of more than about 13 hours.  flags: shz_scan_batch's, and
 * SHZ_SCAN_KEEP_MASK: out_nres[w] holds ON ENTRY a keep mask of the cap_windows windows (recording-major, as a scan of the
 * same arguments orders them) -- a window whose entry is 0 has its out_nres cleared behind the scan and before the timeline,
 * so it is no hit of any segment; its other outputs stay what the scan wrote.  It is how a caller that judged the windows of
 * an earlier scan by a rule of its own (scan(min_score=)) gets the timeline and the zones of the rest. */
int32_t shz_scan_extents(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                         const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                         uint32_t window_frames, uint32_t step_frames, uint32_t topn, uint32_t flags, uint32_t min_aligned,
                         uint32_t max_gap, uint32_t margin_frames, uint32_t d_tol, uint64_t* win_off, uint32_t* out_sid,
                         int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                         uint64_t* out_npairs, uint64_t cap_windows, uint64_t* count, uint32_t* seg_rec, uint32_t* seg_sid,
                         int64_t* seg_shift, uint32_t* seg_first, uint32_t* seg_last, uint32_t* seg_hits, uint32_t* seg_best,
                         uint64_t cap_segs, uint64_t* seg_count, uint32_t* zone_lo, uint32_t* zone_hi, uint32_t* zone_count,
                         uint32_t* zone_q_first, uint32_t* zone_q_last, uint32_t* zone_t_first, uint32_t* zone_t_last,
                         uint32_t* zone_shift, uint32_t* zone_hist, float* ms_extract, float* ms_window, float* ms_match,
                         float* ms_extent);

/* ---- speed-tolerant recognition (new; the reference's hash is an exact (f1, f2, dt) triple, recognizer.py:100-114, so audio
 * played 1 % fast or slow no longer meets the table) ----------------------------------------------------------------------
 * A query that plays s times as fast as the table's copy has its constellation peaks at frequency f s and time t / s.  The
 * spectrogram is left alone: the integer coordinates of the query's peaks are mapped back to the table's domain for every
 * factor of a ladder, and every variant is paired and hashed like generate_hashes (__init__.py:179-210).
 * A factor is Q16: s16 = round(s 65536) in [32768, 131072] (0.5x .. 2x); above 65536 the query plays faster than the table's
 * copy.  For a peak (f, t), in 64-bit integers:
 *     t' = (t s16 + 32768) >> 16        f' = (2 65536 f + s16) / (2 s16)    (integer division: round-half-up of f 65536 / s16)
 * peaks with f' > 2048 leave; the peaks of one (clip, speed) are ordered by (t', f', original index) -- what generate_hashes
 * sees after its stable time sort -- and paired as shz_pair_hash pairs them: each with its next fan_value - 1 successors,
 * 0 <= dt' <= 200, key32 = f1' << 20 | f2' << 8 | dt', t1 = t1'.  At s16 = 65536 the result is shz_pair_hash's, entry for
 * entry.  Numpy twin: tests/speed_twin.py.
 *
 * shz_warp_pair_hash: peaks as for shz_pair_hash ((time asc, freq asc) per clip, t < 2^31; peak_off: n_clips + 1, HOST;
 * peak_f / peak_t host, or device with SHZ_IN_DEVICE -- a host list that breaks the order is SHZ_E_INVALID, a device list is
 * the caller's promise).  Query q owns the adjacent clips [query_clip0[q], query_clip0[q + 1]) as in shz_recognize_batch;
 * query_clip0 = NULL: every clip is a query of its own (n_queries is not read).  OUTPUT ORDER: for query q, for speed v, for
 * every clip c of q, the hashes of (c, v) in generation order -- (q, v) is one contiguous query of the match.  hash_off
 * (HOST, n_clips n_speeds + 1 entries, may be NULL) is the CSR of those segments in that order, exact: the hashes are
 * counted before they are written.  key32 / t1: host, or device with SHZ_OUT_DEVICE; more than cap hashes: SHZ_E_CAPACITY,
 * *count = required, hash_off written, nothing else.  SHZ_E_INVALID before anything is launched: n_speeds of 0 or above 1024,
 * a factor outside the range, fan_value outside [1, 64], a peak_off or query_clip0 that is not a CSR.  SHZ_E_UNSUPPORTED:
 * peaks x speeds x (fan_value - 1) of 2^32 or more in one call. */
int32_t shz_warp_pair_hash(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                           uint32_t n_clips, const uint32_t* query_clip0, uint32_t n_queries, const uint32_t* speed_q16,
                           uint32_t n_speeds, uint32_t fan_value, uint32_t flags, uint32_t* key32, uint32_t* t1,
                           uint64_t* hash_off, uint64_t cap, uint64_t* count);
/* recognize() at an unknown speed: shz_peaks into buffers of the library, the warp above for every factor of speed_q16, and
 * ONE match over n_queries x n_speeds queries ((q, v) = the union over q's channels of variant v); peaks and hashes never
 * visit the host.  Clips, query_clip0, fs, amp_min, fan_value, topn as for shz_recognize_batch; flags: SHZ_PCM_DEVICE,
 * SHZ_MATCH_FULL_SORT.  Per query the BEST variant is the one with the greatest rank-0 aligned count (0 without results);
 * ties go to the factor nearest 65536, then to the lower index.  Outputs (host): out_best[n_queries] = its index into
 * speed_q16; out_sid / out_delta / out_aligned / out_dedup [n_queries topn], out_nres, out_nhash (may be NULL) [n_queries]:
 * the best variant's, shaped as shz_recognize_batch's -- out_delta is in the TABLE's frames; out_profile (may be NULL)
 * [n_queries n_speeds]: the rank-0 aligned count of every variant.  The match's bias bound is the largest warped time,
 * round((max_frames - 1) s_max).  Refused before anything is launched: what shz_recognize_batch refuses, n_speeds of 0 or
 * above 1024 and a factor outside the range (SHZ_E_INVALID), a clip whose warped time could reach 2^20, the query offsets of
 * the match (SHZ_E_UNSUPPORTED).  Queries x speeds go to the warp and the match in slices of whole queries whose hashes stay
 * within the match's 2^28-pair budget and 1/8 of the workspace limit; results do not depend on the slicing
 * (SHZ_DEBUG_SPEED_SMALL_SLICES).  ms_extract / ms_warp / ms_match (may be NULL): hipEvent times of the peak extraction, of
 * the warp stages (with their one read-back a slice) and of the matches. */
int32_t shz_recognize_speeds(shz_ctx* ctx, shz_table* table, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                             const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min, uint32_t fan_value,
                             uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds, uint32_t flags, uint32_t* out_best,
                             uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                             uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, float* ms_extract, float* ms_warp,
                             float* ms_match);

/* ---- two warp factors (new): a time-stretch that keeps the pitch (a DJ deck with key-lock), a pitch shift that keeps the
 * tempo, or both by different amounts move a query's peaks to (f p, t / a) with a tempo factor a and a pitch factor p of their
 * own, which no rung of a speed ladder describes.  A WARP is a pair of Q16 factors (t16, f16), each in [32768, 131072]: the
 * query runs t16 / 65536 times as fast and sounds f16 / 65536 times as high as the table's copy.  The maps are the ones
 * above, each with its own factor:
 *     t' = (t t16 + 32768) >> 16        f' = (2 65536 f + f16) / (2 f16)
 * peaks with f' > 2048 leave, the kept peaks of one (clip, warp) are ordered by (t', f', original index) and paired as
 * above.  Warp v is (tempo_q16[v], pitch_q16[v]); a speed s16 is the warp (s16, s16).  Numpy twin: tests/warp_twin.py.
 *
 * shz_warp_pair_hash_tf: the contract and the output order of shz_warp_pair_hash with "speed v" read as "warp v" (hash_off:
 * n_clips n_warps + 1 entries).  SHZ_E_INVALID before anything is launched: n_warps of 0 or above 1024, a NULL table, a factor
 * of either table outside the range (the message names the table and the index).  shz_warp_pair_hash(speed_q16) is this call
 * with the one table given twice. */
int32_t shz_warp_pair_hash_tf(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                              uint32_t n_clips, const uint32_t* query_clip0, uint32_t n_queries, const uint32_t* tempo_q16,
                              const uint32_t* pitch_q16, uint32_t n_warps, uint32_t fan_value, uint32_t flags, uint32_t* key32,
                              uint32_t* t1, uint64_t* hash_off, uint64_t cap, uint64_t* count);
/* shz_recognize_speeds over warps: the same stages, outputs (out_best: index into the warps; out_profile [n_queries n_warps])
 * and refusals.  The BEST variant is the one with the greatest rank-0 aligned count; ties go to the smaller
 * |t16 - 65536| + |f16 - 65536|, then to the lower index (on a diagonal list: the rule of shz_recognize_speeds).  The bias
 * bound of the match and the t' < 2^20 refusal use the largest t16.  shz_recognize_speeds(speed_q16) is this call with the one
 * table given twice. */
int32_t shz_recognize_warps(shz_ctx* ctx, shz_table* table, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                            const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min, uint32_t fan_value,
                            uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags,
                            uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                            uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, float* ms_extract, float* ms_warp,
                            float* ms_match);
/* shz_recognize_warps with the extent pass of shz_match_extents_fit on every query's results (new).  The warped hashes of a
 * query exist on the device only, so the pass runs inside the call: on every slice of queries, between its match and the
 * next slice's warp.  The arguments of shz_recognize_warps, then drift_bins and the extent outputs (host).  The recognition
 * outputs equal shz_recognize_warps' on the same inputs, entry for entry.  The QUERY of the extent pass for query q is the hash
 * list of its BEST variant -- the union over its channels, as the match saw it --, and candidate n < out_nres[q] is
 * (out_sid[q, n], out_delta[q, n] - w, out_delta[q, n] + w) with w = the context's vote tolerance + drift_bins; ncand = topn.
 * out_count / out_q_first / out_q_last / out_t_first / out_t_last / out_sum_q / out_sum_u / out_sum_qq / out_sum_qu
 * [n_queries topn], out_hist [n_queries topn 64] (may be NULL), out_shift [n_queries]: as shz_match_extents_fit defines them,
 * zero at and past out_nres[q].  out_q_first / out_q_last, the histogram and the shift are in WARPED frames, the table's
 * domain, as out_delta is; the sums' q likewise, and u = d - (out_delta - w).  At tolerance 0 and drift_bins 0, out_count ==
 * out_aligned.  A query whose true tempo a differs from its best rung's lets d = off - t' drift along t' with slope
 * a / rung - 1: drift_bins widens the candidates so that the drifting pairs belong, and the sums give the slope.
 * Refused before anything is launched: what shz_recognize_warps refuses; what shz_match_extents refuses about the table; a
 * NULL extent array other than out_hist, topn > 64 (SHZ_E_INVALID); 2 w + 1 > 4096 (SHZ_E_UNSUPPORTED).  The outputs are
 * written only by a call that returns SHZ_OK.  Results depend neither on the slicing nor on the extent pass's tiling
 * (SHZ_DEBUG_SPEED_SMALL_SLICES, SHZ_DEBUG_EXTENT_SMALL_TILES).  ms_extent (may be NULL): the hipEvent time of the extent
 * stages, the packing of the best variants' hashes included. */
int32_t shz_recognize_warps_extents(shz_ctx* ctx, shz_table* table, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                    const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min,
                                    uint32_t fan_value, uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16,
                                    uint32_t n_warps, uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                                    uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                    uint32_t* out_profile, float* ms_extract, float* ms_warp, float* ms_match, uint32_t drift_bins,
                                    uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first,
                                    uint32_t* out_t_last, uint64_t* out_sum_q, uint64_t* out_sum_u, uint64_t* out_sum_qq,
                                    uint64_t* out_sum_qu, uint32_t* out_hist, uint32_t* out_shift, float* ms_extent);
/* shz_recognize_warps_extents with the one table speed_q16 for time and frequency (as shz_recognize_speeds is to
 * shz_recognize_warps; what is refused about the ladder names n_speeds / speed) */
int32_t shz_recognize_speeds_extents(shz_ctx* ctx, shz_table* table, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                     const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min,
                                     uint32_t fan_value, uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds,
                                     uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                                     uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                     uint32_t* out_profile, float* ms_extract, float* ms_warp, float* ms_match, uint32_t drift_bins,
                                     uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first,
                                     uint32_t* out_t_last, uint64_t* out_sum_q, uint64_t* out_sum_u, uint64_t* out_sum_qq,
                                     uint64_t* out_sum_qu, uint32_t* out_hist, uint32_t* out_shift, float* ms_extent);

/* ---- scanning at an unknown speed (new; shz_scan_batch and shz_recognize_speeds joined: "which songs play in this hour of
 * broadcast, and when?" where the station pitches its songs up or down) --------------------------------------------------
 * shz_scan_speeds: the arguments of shz_scan_batch plus a ladder (speed_q16 / n_speeds, checked as shz_recognize_speeds
 * checks them).  Every recording's peaks are extracted ONCE (shz_peaks), warped, re-ordered and paired for every rung as
 * shz_warp_pair_hash does with the recording as the query, and the warped lists are cut into the windows on the device.
 * WINDOW COUNT: in the recording's own frames, exactly shz_scan_window_count(F_r, window_frames, step_frames); win_off,
 * cap_windows, *count and SHZ_E_CAPACITY as in shz_scan_batch (the total follows from the frame counts alone).
 * WINDOW CONTENTS: with W_v(x) = (x s16 + 32768) >> 16 for rung v (64-bit; the warp's time map), window w starts at recording
 * frame s = w step_frames; its query at rung v is the union, over the recording's channels, of the entries (key32, t1') of
 * (recording, v, channel) with W_v(s) <= t1' < W_v(s + window_frames), and an entry's query offset is t1' - W_v(s).  At s16 =
 * 65536 that is shz_scan_batch's window, entry for entry.  The EDGES note of shz_scan_batch holds here too.
 * MATCH: every (window, rung) is one query of the match on device columns; its bias bound is ceil(window_frames s_max / 65536)
 * - 1, which W_v(s + window_frames) - W_v(s) - 1 never exceeds at any rung or start (at 65536 alone: window_frames - 1).
 * OUTPUTS per window (host, windows recording-major): out_best[n_wins] = the index of the best rung -- greatest rank-0
 * aligned count (0 without results), ties to the factor nearest 65536, then to the lower index; out_sid / out_delta /
 * out_aligned / out_dedup [n_wins topn], out_nres, out_nhash, out_npairs (the last two may be NULL) [n_wins]: the best rung's,
 * shaped as shz_scan_batch's.  out_delta is in the TABLE's frames: the song frame that lies at the window's start.
 * out_profile (may be NULL) [n_wins n_speeds]: the rank-0 aligned count of every rung.
 * REFUSED before anything is launched: everything shz_scan_batch refuses; n_speeds of 0 or above 1024, a factor outside
 * [32768, 131072], fan_value outside [1, 64] (SHZ_E_INVALID); ceil(window_frames s_max / 65536) >= 2^20, the query offsets of
 * the match (SHZ_E_UNSUPPORTED).  A single (recording, rung) whose peaks x (fan_value - 1) reach 2^32, the warp's 32-bit
 * scans, is SHZ_E_UNSUPPORTED too; the peaks are counted by the extraction, so this one comes after it and before any warp.
 * SLICES: the work goes in slices of (whole recordings x a contiguous chunk of rungs) whose warped hashes stay within the
 * match's 2^28-pair budget and 1/8 of the workspace limit (the ladder is cut only where one recording at all rungs is beyond
 * that); inside a slice the windows go to the match in groups as in shz_scan_batch, a window with all its rungs never split;
 * the best rung is folded over the chunks on the host.  Results do not depend on any of it
 * (SHZ_DEBUG_SCAN_SPEED_SMALL_SLICES).  ms_extract / ms_warp / ms_window / ms_match (may be NULL): hipEvent times of the peak
 * extraction, of the warp stages (with their one read-back a slice), of cutting the windows (bounds, scan, read-back,
 * gathers) and of the matches. */
int32_t shz_scan_speeds(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                        const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                        uint32_t window_frames, uint32_t step_frames, uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds,
                        uint32_t flags, uint64_t* win_off, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                        uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                        uint32_t* out_profile, uint64_t cap_windows, uint64_t* count, float* ms_extract, float* ms_warp,
                        float* ms_window, float* ms_match);
/* The timeline of a speed-tolerant scan (no GPU, no ctx).  shz_scan_timeline's identity shift = delta - w step_frames is
 * not constant when the recording plays faster or slower than the table's copy (at 1.03 the song advances 22 or 23 frames a
 * 22-frame step), and neighbouring windows may choose neighbouring rungs, so continuity is judged between neighbouring hits.
 * Inputs: win_off and out_sid / out_delta / out_aligned (stride topn, rank 0 is read) / out_nres / out_best of
 * shz_scan_speeds, and its ladder (rung_tol compares INDICES: hand over a sorted ladder).  A window is a HIT iff nres >= 1
 * and its rank-0 aligned >= min_aligned.  The windows of a recording are visited in order with one open segment, whose last
 * hit is w1 with rung v1 and delta1: a hit w2 (rung v2, delta2) CONTINUES it iff the song id is the same, w2 - w1 - 1 <=
 * max_gap, |v2 - v1| <= rung_tol and |delta2 - delta1 - W_v2((w2 - w1) step_frames)| <= shift_tol (W_v as above, 64-bit);
 * any other hit closes it and opens a new one; a window without a hit changes nothing; the recording's end closes it.
 * Per segment (recording-major, in order): recording, sid, first and last window, hit windows, largest aligned count,
 * pos_first / pos_last (the deltas of its first and last hit: song frames at those windows' starts), and seg_rung = the
 * index of the rung its hits chose most often (ties to the factor nearest 65536, then to the lower index).  Two-call idiom
 * as shz_scan_timeline: more than cap segments: SHZ_E_CAPACITY, *count = their number, the first cap are written (cap = 0:
 * the seg_* pointers may be NULL).  SHZ_E_INVALID: a ladder shz_scan_speeds would refuse, an out_best entry >= n_speeds,
 * topn of 0, a win_off that decreases. */
int32_t shz_scan_timeline_speeds(const uint64_t* win_off, uint32_t n_recs, const uint32_t* out_sid, const int32_t* out_delta,
                                 const uint32_t* out_aligned, const uint32_t* out_nres, const uint32_t* out_best, uint32_t topn,
                                 uint32_t step_frames, const uint32_t* speed_q16, uint32_t n_speeds, uint32_t min_aligned,
                                 uint32_t max_gap, uint32_t rung_tol, uint32_t shift_tol, uint32_t* seg_rec, uint32_t* seg_sid,
                                 uint32_t* seg_first, uint32_t* seg_last, uint32_t* seg_hits, uint32_t* seg_best,
                                 int32_t* seg_pos_first, int32_t* seg_pos_last, uint32_t* seg_rung, uint64_t cap, uint64_t* count);

/* ---- scanning at unknown tempo and pitch, per-window variant lists (new; shz_scan_speeds over warp pairs: DESIGN.md 3.7i) ----
 * shz_scan_warps: the arguments of shz_scan_speeds with the ladder replaced by a warp list (tempo_q16 / pitch_q16 / n_warps,
 * checked as shz_recognize_warps checks them: the message names the table and the index), an optional selection (sel_off /
 * sel_warp, host) and an optional out_work[2].
 * DENSE (both selection pointers NULL): the contract of shz_scan_speeds with "rung v" read as "warp v".  The hashes of
 * (recording, warp, channel) are shz_warp_pair_hash_tf's.  Only the TIME factor enters a time: W_v(x) = (x t16 + 32768) >> 16
 * gives the window borders and the query offsets, the bias bound of the match is ceil(window_frames t16_max / 65536) - 1, and
 * ceil(window_frames t16_max / 65536) >= 2^20 is SHZ_E_UNSUPPORTED; pitch_q16 never enters a time.  The BEST variant of a
 * window has the greatest rank-0 aligned count; ties go to the smaller |t16 - 65536| + |f16 - 65536|, then to the lower index.
 * out_profile (may be NULL) is [n_wins n_warps].  shz_scan_speeds(speed_q16) is this call with the one table given twice and
 * no selection.
 * SELECTION: sel_off has n_wins + 1 entries over the windows, recording-major as in win_off (the caller knows n_wins from
 * shz_scan_window_count), and sel_warp[sel_off[w] .. sel_off[w + 1]) are the warps window w tries, strictly ascending, each
 * < n_warps.  Only the listed (window, warp) pairs become queries of the match.  out_profile is slot-aligned (sel_off[n_wins]
 * entries), the best variant is chosen among the window's slots by the rule above, and a window with an empty list has nres
 * 0, all arrays 0 and out_best = SHZ_SCAN_NO_WARP.  Warps that no window selects are dropped before slicing, and from there
 * the call behaves as on the compacted list; if nothing is selected, nothing is extracted.  A full selection (every window
 * lists 0 .. n_warps - 1) gives the dense call's arrays, entry for entry.  SHZ_E_INVALID before anything is launched: exactly
 * one of the two pointers NULL, sel_off[0] != 0, a sel_off that decreases, a list that is not strictly ascending, an index
 * >= n_warps.
 * out_work (may be NULL): [0] = the warped hash entries written over the call (the sum of the slices' CSR totals), [1] = the
 * window entries handed to the match (the sum of the window stage's totals): what a selection saves, as counts.
 * SLICES as in shz_scan_speeds; a chunk of warps may cut through a window's list, and the best variant is folded over the
 * chunks in index order.  Results do not depend on any of it (SHZ_DEBUG_SCAN_SPEED_SMALL_SLICES: 1 recording x 2 warps a
 * slice, 3 windows a group). */
#define SHZ_SCAN_NO_WARP 0xFFFFFFFFu
int32_t shz_scan_warps(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                       const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                       uint32_t window_frames, uint32_t step_frames, uint32_t topn, const uint32_t* tempo_q16,
                       const uint32_t* pitch_q16, uint32_t n_warps, const uint64_t* sel_off, const uint32_t* sel_warp,
                       uint32_t flags, uint64_t* win_off, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                       uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                       uint32_t* out_profile, uint64_t* out_work, uint64_t cap_windows, uint64_t* count, float* ms_extract,
                       float* ms_warp, float* ms_window, float* ms_match);
/* The timeline of a scan over warps (no GPU, no ctx): shz_scan_timeline_speeds over a warp list that need not be sorted (any
 * length >= 1, every factor in [32768, 131072]).  A hit w2 (warp (t2, f2), delta2) CONTINUES the open segment, whose last hit
 * is w1 (warp (t1, f1), delta1), iff the song id is the same, w2 - w1 - 1 <= max_gap, |t2 - t1| <= tempo_tol_q16, |f2 - f1| <=
 * pitch_tol_q16 and |delta2 - delta1 - W_t2((w2 - w1) step_frames)| <= shift_tol.  out_best is read for hits only, so
 * SHZ_SCAN_NO_WARP on a window without results is fine (on a hit, an entry >= n_warps is SHZ_E_INVALID).  Per segment the
 * arrays of the speed timeline, with seg_warp = the variant its hits chose most often (ties to the smaller
 * |t16 - 65536| + |f16 - 65536|, then to the lower index).  Capacity: the same two-call idiom. */
int32_t shz_scan_timeline_warps(const uint64_t* win_off, uint32_t n_recs, const uint32_t* out_sid, const int32_t* out_delta,
                                const uint32_t* out_aligned, const uint32_t* out_nres, const uint32_t* out_best, uint32_t topn,
                                uint32_t step_frames, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps,
                                uint32_t min_aligned, uint32_t max_gap, uint32_t tempo_tol_q16, uint32_t pitch_tol_q16,
                                uint32_t shift_tol, uint32_t* seg_rec, uint32_t* seg_sid, uint32_t* seg_first, uint32_t* seg_last,
                                uint32_t* seg_hits, uint32_t* seg_best, int32_t* seg_pos_first, int32_t* seg_pos_last,
                                uint32_t* seg_warp, uint64_t cap, uint64_t* count);

/* ---- warped scan extents (new): frame-accurate play bounds and a tempo fit for every segment of a speed-,
 * tempo- or pitch-tolerant scan.  shz_scan_extents serves the plain scan, whose segments have one constant shift.  A segment of
 * shz_scan_timeline_speeds / _warps has none: the recording plays at a tempo of its own, the rung its windows chose is only
 * near it, and the offset difference DRIFTS over the play.  So every segment brings its own pair (t16, f16) -- Q16 VALUES, not
 * indices, which serves ladders, pair lists, chunked grids and the separable search alike (a speed is t16 == f16) --, its zones
 * are cut from hash lists warped at that pair, and the candidate of a zone is widened by drift_bins and comes back with the
 * four moments of shz_match_extents_fit, from which the host fits the tempo the play really runs at.
 * For segment i: recording r, song sid, first / last window a, b, p_a = seg_pos_first, p_b = seg_pos_last (the song frames at
 * the starts of those windows, as the warped timelines emit them), W = window_frames, S = step_frames, M = margin_frames and
 * W(x) = (x t16 + 32768) >> 16 in 64 bits.
 * ZONES (shz_scan_play_zones; no GPU, no ctx; tests/scan_play_twin.py is the same in Python): zone_lo / zone_hi, in the
 * recording's OWN frames, are exactly what shz_scan_zones gives for these segments with every seg_shift 0 -- a warped play has
 * no constant shift, so the identity that keeps margins out of each other's windows is (rec, sid).  Zone z of segment i sits at
 * 3 i + z: whole, head, tail.  zone_wlo / zone_whi are their warped borders W(lo), W(hi) (64 bits: F < 2^32 at factor 2).
 * A zone's QUERY is the union, over the recording's channels, of the entries (key32, t1') of shz_warp_pair_hash_tf's list for
 * (channel, (t16, f16)) with W(lo) <= t1' < W(hi), at query offset t1' - W(lo): the window contents of shz_scan_warps with
 * arbitrary borders (EDGES at shz_scan_batch apply).  This is the definition; the twin computes it from the full warped list
 * of the whole channel.
 * A zone's one CANDIDATE, in 64-bit signed arithmetic, with c_a = p_a - W(a S) + W(lo), c_b = p_b - W(b S) + W(lo) and
 * w = the vote tolerance + drift_bins:
 *   0 whole  (sid, min(c_a, c_b) - w, max(c_a, c_b) + w)     the drift line runs from one end to the other
 *   1 head   (sid, c_a - w, c_a + w)
 *   2 tail   (sid, c_b - w, c_b + w)
 * A range that lies wholly outside int32 is NO candidate (cand_n = 0, d_lo = d_hi = 0); the others are clamped to int32, which
 * loses no pair (shz_scan_extents' argument).  (a S and b S saturate at 2^40 like shz_scan_zones' positions; such a range lies
 * below int32 whatever the rest is.)
 * shz_scan_play_zones writes zone_lo, zone_hi, zone_wlo, zone_whi, zone_d_lo, zone_d_hi and cand_n, [3 n_segs] each, and only
 * when it returns SHZ_OK.  n_segs = 0: SHZ_OK.  Refused, in this order: what shz_scan_zones refuses (SHZ_E_INVALID); a NULL
 * array with n_segs > 0 (SHZ_E_INVALID); a seg_t16 outside [32768, 131072] (SHZ_E_INVALID); a zone with W(hi) - W(lo) >= 2^20
 * (a query offset of the extent pass; SHZ_E_UNSUPPORTED); a used candidate with d_hi - d_lo >= 4096 (the moments;
 * SHZ_E_UNSUPPORTED).  With t16 = 65536, p_a = shift + a S, p_b = shift + b S and w = d_tol, and no song with segments at two
 * shifts in one recording, zones and candidates are shz_scan_zones' and shz_scan_extents'. */
int32_t shz_scan_play_zones(const uint32_t* seg_rec, const uint32_t* seg_sid, const uint32_t* seg_first, const uint32_t* seg_last,
                            const int32_t* seg_pos_first, const int32_t* seg_pos_last, const uint32_t* seg_t16, uint64_t n_segs,
                            const uint64_t* frames, uint32_t n_recs, uint32_t window_frames, uint32_t step_frames,
                            uint32_t margin_frames, uint32_t w, uint32_t* zone_lo, uint32_t* zone_hi, uint64_t* zone_wlo,
                            uint64_t* zone_whi, int32_t* zone_d_lo, int32_t* zone_d_hi, uint32_t* cand_n);
/* The device stage, for the segments a caller folded from any warped scan of the same audio.  pcm .. step_frames and flags
 * (SHZ_PCM_DEVICE) are shz_scan_warps'; seg_* [n_segs] are the caller's segments in the timeline's order, each with its pair.
 * Stages: (a) the peaks of every clip, once; (b) one JOB per (segment, channel): the channel's peaks whose warped time lies in
 * [W(lo0), W(hi0) - 1 + 200] ([lo0, hi0) = zone 0; 200 = the largest dt of a hash), found by two warped-time binary searches
 * on the device -- whole t' groups, and every partner of every anchor below W(hi0), so the job's hashes with t1' < W(hi0) are
 * the full list's, entry for entry; (c) the warp stage of shz_warp_pair_hash_tf on the jobs, every item taking its factors and
 * its peak range from its job; (d) the three zones of every segment cut from its jobs' hash lists at W(lo), W(hi); (e) the
 * extent pass with the moments, one candidate a zone.  Only the plays are warped, each at its own pair -- about one recording's
 * peaks, where warping whole recordings at every pair in use costs (pairs in use) x the recording.  Warped hashes never leave
 * the device.  The unsharded table only.
 * Outputs, [3 n_segs] each, zone z of segment i at 3 i + z: zone_lo / zone_hi / zone_d_lo / zone_d_hi (shz_scan_play_zones'),
 * zone_count, zone_q_first / zone_q_last (in WARPED recording frames: offset + W(lo), where count > 0; 0 otherwise),
 * zone_t_first / zone_t_last (song frames), zone_shift, zone_hist [x 64, bucket (t1' - W(lo)) >> shift; may be NULL] and
 * zone_sum_q / _u / _qq / _qu: the RESULT of shz_match_extents_fit for the zone's query and candidate (q = the query offset,
 * u = d - zone_d_lo).  out_work (may be NULL): [0] peak items warped, [1] hash entries written, [2] zone entries handed to the
 * extent pass.  ms_extract / ms_warp (jobs and warp) / ms_extent (cut and extent pass): hipEvent times, may be NULL.  Every
 * output is written only by a call that returns SHZ_OK.  n_segs = 0: SHZ_OK, nothing is launched, nothing is written.  Results
 * depend neither on the extent pass's tiling nor on anything else (SHZ_DEBUG_EXTENT_SMALL_TILES).
 * Refused before anything is launched, in this order: flags beyond SHZ_PCM_DEVICE, window_frames outside [1, 2^20),
 * step_frames of 0, fan_value outside [1, 64], margin_frames >= 2^20 (SHZ_E_INVALID); [n_segs = 0 returns here]; 3 n_segs >=
 * 2^31 (SHZ_E_UNSUPPORTED); no recording, rec_clip0 / clip_off as shz_scan_warps refuses them, Fs of 0, a NULL pcm, a NULL
 * segment or zone array, a seg_f16 outside [32768, 131072] (SHZ_E_INVALID); the table as shz_match_extents refuses it; then
 * what shz_scan_play_zones refuses, with w = the context's vote tolerance + drift_bins; a warped border >= 2^32
 * (SHZ_E_UNSUPPORTED).  Seen on the device: 2^32 or more (peak item, partner) pairs in the one pass (SHZ_E_UNSUPPORTED). */
int32_t shz_scan_plays(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                       const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                       uint32_t window_frames, uint32_t step_frames, uint32_t flags, const uint32_t* seg_rec,
                       const uint32_t* seg_sid, const uint32_t* seg_first, const uint32_t* seg_last, const int32_t* seg_pos_first,
                       const int32_t* seg_pos_last, const uint32_t* seg_t16, const uint32_t* seg_f16, uint64_t n_segs,
                       uint32_t margin_frames, uint32_t drift_bins, uint32_t* zone_lo, uint32_t* zone_hi, int32_t* zone_d_lo,
                       int32_t* zone_d_hi, uint32_t* zone_count, uint32_t* zone_q_first, uint32_t* zone_q_last,
                       uint32_t* zone_t_first, uint32_t* zone_t_last, uint32_t* zone_shift, uint32_t* zone_hist,
                       uint64_t* zone_sum_q, uint64_t* zone_sum_u, uint64_t* zone_sum_qq, uint64_t* zone_sum_qu,
                       uint64_t* out_work, float* ms_extract, float* ms_warp, float* ms_extent);

/* ---- repeated content inside a recording (new; no table, no catalogue) -------------------------------------------------
 * "Which stretches of this recording air more than once?" -- adverts, jingles, idents, a song nobody has inserted yet.  Two
 * hashes of one recording with the same key at times t_i < t_j vote for the lag t_j - t_i; a stretch that airs twice piles
 * its votes on one lag over a contiguous stretch of t_i (tests/repeat_twin.py is the definition in Python).
 * All quantities are integers, in frames at the ctx's hop.
 * HASHES: recording r owns the adjacent clips (its channels) [rec_clip0[r], rec_clip0[r + 1]), as in shz_scan_batch; H_r is
 * the SET of (key32, t1) over its channels.  rec_hashes[r] = |H_r|.
 * PAIRS: per key of H_r with the distinct times t_0 < ... < t_(m-1): m > max_run is a stop hash -- no pairs, 1 to
 * rec_skipped_keys[r], m to rec_skipped_rows[r]; otherwise every i < j with min_lag <= t_j - t_i <= max_lag is the pair
 * (lag = t_j - t_i, t = t_i).  Pairs never cross recordings.  rec_pairs[r] = their number.
 * CELLS: (r, lag, block = t >> cell_shift) with pairs (count), first (min t) and last (max t).  Returned: the cells with
 * pairs >= min_cell_pairs in the order (r, lag, block) ascending -- cell_lag / _block / _pairs / _first / _last [cap_cells] --
 * and cell_off[n_recs + 1], their CSR over the recordings.  More than cap_cells: SHZ_E_CAPACITY, *count = the cells needed;
 * cell_off and the four rec_* arrays are filled all the same, and the first cap_cells cells written.
 * The device chain, all integer: compose rec << 52 | key32 << 20 | t1; sort on the significant bits, unique; runs (one key
 * of one recording); partners of every element by two binary searches inside its run; a 64-bit scan; pair keys rec << 40 |
 * lag << 20 | t written by output tile; sort on the bits from cell_shift up; cell heads, exact min / max, compaction.
 * Recordings go through the pair stage in slices of consecutive whole recordings whose two pair buffers fit 1/8 of the
 * workspace limit (shz_set_workspace_limit); the results do not depend on the slicing (SHZ_DEBUG_REPEAT_SMALL_SLICES).  A
 * single recording whose pairs do not fit is SHZ_E_UNSUPPORTED: the message names it, its pairs and the two knobs, min_lag
 * and max_run.  More than 4,096 recordings in one call, or 2^32 hashes or more: SHZ_E_UNSUPPORTED.
 * Refused before anything is launched, nothing written (SHZ_E_INVALID): a NULL ctx, count, cell_off or rec_* array, a NULL
 * cell array with cap_cells > 0, a NULL column with hashes; clips without a recording, rec_clip0 / hash_off / clip_off that
 * do not start at 0, decrease or do not end at n_clips; unknown flag bits; max_lag < min_lag; max_lag >= 2^20; max_run
 * outside [2, 1024]; cell_shift > 19; min_cell_pairs of 0; (shz_repeats_hashes) a t1 >= 2^20; (shz_repeats_batch) fan_value
 * outside [1, 64].  n_recs = 0 or no hashes: SHZ_OK, no cells, cell_off all 0.
 * shz_repeats_hashes: key32 / t1 are HOST columns, hash_off[n_clips + 1] their CSR over the clips; they are copied into
 * device buffers the call allocates and frees (tests / tools, as shz_match_device_host).  flags: 0.
 * shz_repeats_batch: the clips are fingerprinted into the library's own buffers (as shz_scan_batch: pcm host, or device with
 * SHZ_PCM_DEVICE) and the chain reads them there -- no hash crosses the bus.  ms_extract / ms_pairs / ms_cells (may be NULL):
 * hipEvent intervals of the extraction, of compose .. expand and of the cell stage.  They are intervals on the stream, not
 * kernel time alone: the host read-backs inside a stage (the unique count and the recordings' numbers in ms_pairs; per
 * slice the cell count, the kept count and the copy of the cells in ms_cells) and their synchronisations lie inside them.
 * They are written (0 first) only once nothing more can be refused before a launch. */
int32_t shz_repeats_hashes(shz_ctx* ctx, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off, uint32_t n_clips,
                           const uint32_t* rec_clip0, uint32_t n_recs, uint32_t min_lag, uint32_t max_lag, uint32_t max_run,
                           uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag,
                           uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last,
                           uint32_t* rec_hashes, uint32_t* rec_skipped_keys, uint64_t* rec_pairs, uint64_t* rec_skipped_rows,
                           uint64_t cap_cells, uint64_t* count);
int32_t shz_repeats_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* rec_clip0,
                          uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value, uint32_t min_lag, uint32_t max_lag,
                          uint32_t max_run, uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off,
                          uint32_t* cell_lag, uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first,
                          uint32_t* cell_last, uint32_t* rec_hashes, uint32_t* rec_skipped_keys, uint64_t* rec_pairs,
                          uint64_t* rec_skipped_rows, uint64_t cap_cells, uint64_t* count, float* ms_extract, float* ms_pairs,
                          float* ms_cells);
/* The fold (no GPU, no ctx): the returned cells of every recording joined into repeats.  Two cells of one recording are
 * LINKED iff |lag - lag'| <= lag_tol and |block - block'| <= max_gap + 1; a repeat is a connected component of that relation
 * whose summed pairs reach min_pairs.  Per repeat: rec; lag = the lag holding the most pairs of the component (the smaller
 * on a tie); lag_lo / lag_hi; first (min) and last (max) over its cells; pairs (64 bits); cells.  The audio of [first, last]
 * airs again at [first + lag, last + lag].  Order: (rec, first, lag, smallest cell index of the component) ascending.  Each
 * cell looks its neighbours up in the sorted list (union-find over cell indices): no pass over all pairs of cells.  Two-call
 * idiom as shz_scan_timeline: more than cap repeats: SHZ_E_CAPACITY, *count = their number, the first cap are written (cap =
 * 0: the rep_* pointers may be NULL).  SHZ_E_INVALID: a NULL count, cell_off (which must start at 0 and not decrease) or, with
 * cells, a NULL cell array; a NULL rep_* array with cap > 0; cells of a recording that are not in strictly ascending (lag,
 * block) order; a cell whose first > last. */
int32_t shz_repeats_fold(const uint64_t* cell_off, uint32_t n_recs, const uint32_t* cell_lag, const uint32_t* cell_block,
                         const uint32_t* cell_pairs, const uint32_t* cell_first, const uint32_t* cell_last, uint32_t lag_tol,
                         uint32_t max_gap, uint64_t min_pairs, uint32_t* rep_rec, uint32_t* rep_lag, uint32_t* rep_lag_lo,
                         uint32_t* rep_lag_hi, uint32_t* rep_first, uint32_t* rep_last, uint64_t* rep_pairs, uint32_t* rep_cells,
                         uint64_t cap, uint64_t* count);

/* ---- content shared between recordings (new; no table, no catalogue) -----------------------------------------------------
 * "Which stretches of recording a also air in recording b?" -- station A against station B, Monday's adverts against
 * Tuesday's, one unlabelled tape against another, the night half of a day against its day half.  The join of
 * shz_repeats_* between TWO recordings with a SIGNED lag, driven by a list of jobs (tests/shared_twin.py
 * is the definition in Python).  All quantities are integers, in frames at the ctx's hop.
 * HASHES: recordings, clips and H_r as in shz_repeats_*.  rec_hashes[r] = |H_r|.
 * JOBS: job j = (job_a[j], job_b[j]), two different recordings < n_recs.  A recording may be named by any number of jobs,
 * (a, b) and (b, a) may both be listed, and a job listed twice is answered twice.
 * PAIRS: per job and key present in H_a and H_b, with m_a distinct times in a and m_b in b: m_a > max_run or m_b > max_run
 * is a stop hash -- no pairs, 1 to job_skipped_keys[j], m_a + m_b to job_skipped_rows[j]; otherwise every (t_a, t_b) with
 * lag_lo <= t_b - t_a <= lag_hi is the pair (lag = t_b - t_a, t = t_a).  job_pairs[j] = their number.
 * CELLS: (j, lag, block = t_a >> cell_shift) with pairs, first (min t_a) and last (max t_a).  Returned: the cells with
 * pairs >= min_cell_pairs in the order (j, lag, block) ascending, and cell_off[n_jobs + 1], their CSR over the JOBS.
 * cell_lag is BIASED: lag + SHZ_SHARED_LAG_BIAS, so that the arrays of a call feed shz_repeats_fold as they are, the jobs
 * standing in for its recordings (its order check and its |lag - lag'| <= lag_tol do not see the bias; the caller takes
 * the bias off rep_lag / rep_lag_lo / rep_lag_hi).  The audio of [first, last] in a airs in b at [first + lag, last + lag].
 * More than cap_cells: SHZ_E_CAPACITY, *count = the cells needed; cell_off, rec_hashes and the three job_* arrays are filled
 * all the same, and the first cap_cells cells written.
 * The device chain, all integer: the elements, runs and recording borders of shz_repeats_*; one ITEM per (job, unique
 * element of a); per item the run of its key in b by a lower and an upper bound, and its partners there by two more
 * searches for t_a + lag_lo and t_a + lag_hi (signed, cut to [0, 2^20 - 1]); a 64-bit scan; pair keys job << 41 | (lag +
 * 2^20) << 20 | t_a written by output tile; from there the cell stage of shz_repeats_* on a lag field of 21 bits.  Jobs go
 * through the pair stage in slices of consecutive whole jobs whose two pair buffers fit 1/8 of the workspace limit; the
 * results do not depend on the slicing (SHZ_DEBUG_REPEAT_SMALL_SLICES: one job a slice).  A single job whose pairs do not
 * fit is SHZ_E_UNSUPPORTED: the message names it, its recordings, its pairs, the lag window and max_run.  Also
 * SHZ_E_UNSUPPORTED: more than 4,096 recordings or 4,096 jobs in one call, 2^32 hashes or more, 2^32 items or more.
 * Refused before anything is launched, nothing written (SHZ_E_INVALID): what shz_repeats_* refuses (with job_* in the place
 * of its rec_* arrays), and: a NULL job_a / job_b with n_jobs > 0; a job with a == b or a recording >= n_recs; a lag
 * window outside [-(2^20 - 1), 2^20 - 1]; lag_hi < lag_lo.  n_jobs = 0 or no hashes: SHZ_OK, no cells, cell_off all 0;
 * rec_hashes is filled all the same.
 * shz_shared_hashes: HOST columns, as shz_repeats_hashes (tests / tools).  flags: 0.
 * shz_shared_batch: the clips are fingerprinted into the library's own buffers, as shz_repeats_batch (flags:
 * SHZ_PCM_DEVICE) -- every recording once, whatever the number of jobs that name it, and no hash crosses the bus.
 * ms_extract / ms_pairs / ms_cells as there: stream intervals with the host read-backs of their stage inside them (ms_pairs:
 * the unique count, the recordings' borders, the jobs' numbers). */
#define SHZ_SHARED_LAG_BIAS 1048576u
int32_t shz_shared_hashes(shz_ctx* ctx, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off, uint32_t n_clips,
                          const uint32_t* rec_clip0, uint32_t n_recs, const uint32_t* job_a, const uint32_t* job_b,
                          uint32_t n_jobs, int32_t lag_lo, int32_t lag_hi, uint32_t max_run, uint32_t cell_shift,
                          uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag, uint32_t* cell_block,
                          uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last, uint32_t* rec_hashes,
                          uint64_t* job_pairs, uint32_t* job_skipped_keys, uint64_t* job_skipped_rows, uint64_t cap_cells,
                          uint64_t* count);
int32_t shz_shared_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* rec_clip0,
                         uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value, const uint32_t* job_a,
                         const uint32_t* job_b, uint32_t n_jobs, int32_t lag_lo, int32_t lag_hi, uint32_t max_run,
                         uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag,
                         uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last,
                         uint32_t* rec_hashes, uint64_t* job_pairs, uint32_t* job_skipped_keys, uint64_t* job_skipped_rows,
                         uint64_t cap_cells, uint64_t* count, float* ms_extract, float* ms_pairs, float* ms_cells);

/* ---- ALTERED content shared between recordings (new): the join at a table of warps ------------------------------------------
 * Station B pitches a song up 3 % that station A plays straight; the night re-run of a show comes off a drifting deck; a 25/24
 * video transfer of a tape is compared with the tape.  No catalogue row stands behind either side, and one per cent of speed
 * already empties the plain join (an exact (f1, f2, dt) key).  So the join runs at a table of warps (DESIGN.md 3.7r;
 * tests/shared_warp_twin.py is the definition in Python).  All quantities are integers, in frames at the ctx's hop.
 * WARPS: (tempo_q16[v], pitch_q16[v]), v < n_warps, as shz_warp_pair_hash_tf takes them.
 * HASHES: H_r as in shz_shared_*, formed from r's PEAKS: the entries of one clip are the pairs of its peak list.  H_{r,v}: the
 * same over the peak lists warped by warp v -- exactly the maps, the dropped peaks and the order of shz_warp_pair_hash_tf.  At
 * (65536, 65536) H_{r,v} = H_r.  rec_hashes[r] = |H_r|.
 * JOBS: job j = (job_a[j], job_b[j], job_v[j], job_lag_lo[j], job_lag_hi[j]): what of recording a, played tempo / 65536 times as
 * fast and sounding pitch / 65536 times as high as b's copy, airs in b.  a == b is allowed -- the warped repeat inside one
 * recording; the caller keeps the trivial lags out with the window.  Every job has a window of its own.
 * PAIRS, stop hashes, CELLS, their order, the bias of cell_lag and the capacity idiom: those of shz_shared_*, with H_{a,v} in
 * the place of H_a, H_b plain and the job's window.  t is a's WARPED time t'_a, lag = t_b - t'_a, block = t'_a >> cell_shift.
 * job_hashes[j] = |H_{a,v}|.
 * The chain, all on the ctx's stream: the peaks of every clip once; ONE warp pass in the job form over every
 * clip at (65536, 65536) and the clips of every distinct (a, v) some job names -- ten jobs that name one (a, v) warp it once
 * --, whole peak ranges; the columns go to the join of shz_shared_* as VIRTUAL recordings, r for the plain ones and n_recs + k
 * for the k-th distinct (a, v), with (virtual(a, v), b) as its job; the count kernel reads the window of its job.  No hash
 * leaves the device.  The warp pass is not sliced.
 * Refused before anything is launched, nothing written (SHZ_E_INVALID): what shz_shared_* refuses except a == b; what
 * shz_warp_pair_hash_tf refuses about the table (n_warps in [1, 1024], factors in [32768, 131072]); a job_v >= n_warps; a NULL
 * job array with n_jobs > 0; a window of a job outside [-(2^20 - 1), 2^20 - 1] or with lag_hi < lag_lo (the message names the
 * job).  SHZ_E_UNSUPPORTED, before any launch where it depends on the inputs alone: more than 4,096 jobs; n_recs + distinct (a,
 * v) above 4,096 (a warped recording is a recording of the join); a clip of a whose largest warped time ((frames - 1) t16 +
 * 32768) >> 16 reaches 2^20 (shz_shared_warps_peaks: its last peak's time in the place of frames - 1); 2^32 or more (peak,
 * warp) items times (fan_value - 1), hashes or join items; a job that alone exceeds a slice.  n_jobs = 0 or no peaks: SHZ_OK,
 * no cells, rec_hashes filled.
 * shz_shared_warps_peaks: HOST peak lists (tests / tools), peak_off[n_clips + 1] from 0; the library copies them into device
 * buffers it allocates and frees.  Also SHZ_E_INVALID: a t >= 2^20, an f > 2048, peaks of a clip not in (t asc, f asc) order.
 * flags: 0.
 * shz_shared_warps_batch: PCM (flags: SHZ_PCM_DEVICE).  ms_extract / ms_warp / ms_pairs / ms_cells (each may be NULL): stream
 * intervals with the host read-backs of their stage inside them (ms_warp: the job ranges and the CSR of the pass; the others
 * as shz_shared_batch). */
int32_t shz_shared_warps_peaks(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                               uint32_t n_clips, const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fan_value,
                               const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, const uint32_t* job_a,
                               const uint32_t* job_b, const uint32_t* job_v, const int32_t* job_lag_lo, const int32_t* job_lag_hi,
                               uint32_t n_jobs, uint32_t max_run, uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags,
                               uint64_t* cell_off, uint32_t* cell_lag, uint32_t* cell_block, uint32_t* cell_pairs,
                               uint32_t* cell_first, uint32_t* cell_last, uint32_t* rec_hashes, uint32_t* job_hashes,
                               uint64_t* job_pairs, uint32_t* job_skipped_keys, uint64_t* job_skipped_rows, uint64_t cap_cells,
                               uint64_t* count);
int32_t shz_shared_warps_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                               const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                               const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, const uint32_t* job_a,
                               const uint32_t* job_b, const uint32_t* job_v, const int32_t* job_lag_lo, const int32_t* job_lag_hi,
                               uint32_t n_jobs, uint32_t max_run, uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags,
                               uint64_t* cell_off, uint32_t* cell_lag, uint32_t* cell_block, uint32_t* cell_pairs,
                               uint32_t* cell_first, uint32_t* cell_last, uint32_t* rec_hashes, uint32_t* job_hashes,
                               uint64_t* job_pairs, uint32_t* job_skipped_keys, uint64_t* job_skipped_rows, uint64_t cap_cells,
                               uint64_t* count, float* ms_extract, float* ms_warp, float* ms_pairs, float* ms_cells);

#ifdef __cplusplus
}
#endif
#endif /* SHZ_H */
