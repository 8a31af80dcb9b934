// recognize() for a batch of clips in ONE call (recognizer.py:377-392: fingerprint every channel, union the hashes, match,
// align): the extraction pass writes its hashes into device buffers of the library, the match reads them there -- no
// hash crosses the bus in either direction.
//
// Channels of a query are adjacent clips, so the per-query CSR is a sub-sampling of the extraction's hash_off, which
// is on the host after the extraction's one read-back; the union of the channels' hashes is the sort + unique of the
// match's head.  The queued one-workgroup fold of a single small query needs a bias before the offsets are looked at:
// every t1 of a clip is below its frame count, so the largest frame count - 1 is a bound the host has for free.
#include <algorithm>

#include "shz_internal.h"

// What every fused call refuses about its clips before anything is launched.  clip0 (`name`, for the message) is the CSR of
// the clips over the n items (`what`: queries, recordings): not NULL, starts at 0, ends at n_clips, never decreases
int32_t shz_check_clip0(shz_ctx* ctx, const char* name, const char* what, const uint32_t* clip0, uint32_t n, uint32_t n_clips) {
  if (!clip0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s is NULL", name);
  if (clip0[0] != 0 || clip0[n] != n_clips)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s must start at 0 and end at n_clips = %u (it runs from %u to %u)", name, n_clips, clip0[0], clip0[n]);
  for (uint32_t i = 0; i < n; ++i)
    if (clip0[i + 1] < clip0[i]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s decreases at %s %u", name, what, i);
  return SHZ_OK;
}
int32_t shz_check_clip_off(shz_ctx* ctx, const uint64_t* clip_off, uint32_t n_clips) {
  if (!clip_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "clip_off is NULL");
  for (uint32_t c = 0; c < n_clips; ++c)
    if (clip_off[c + 1] < clip_off[c]) SHZ_FAIL(ctx, SHZ_E_INVALID, "clip_off decreases at clip %u", c);
  return SHZ_OK;
}

// The extraction half of the fused calls (shz_recognize_batch, shz_scan_batch): the hashes go to the slots SHZ_WS_RQ_KEY /
// SHZ_WS_RQ_T1, sized from the frame counts (what the extraction pass itself estimates: 12 peaks a frame with all their
// partners); the pass's SHZ_E_CAPACITY names the size that is enough
int32_t shz_extract_owned(shz_ctx* ctx, const char* who, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                          uint32_t fs, double amp_min, uint32_t fan_value, uint32_t flags, uint64_t* hash_off,
                          const uint32_t** d_key_out, const uint32_t** d_t1_out) {
  *d_key_out = *d_t1_out = nullptr;
  hash_off[0] = 0;
  if (n_clips == 0) return SHZ_OK;
  uint64_t frames = 0;
  for (uint32_t c = 0; c < n_clips; ++c) frames += shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop);
  void *d_key = nullptr, *d_t1 = nullptr;
  uint64_t cap = shz_recognize_estimate(frames, fan_value);
  // (slots that an earlier, larger call has grown are used whole: no pass is repeated for room that is there)
  const uint64_t have = std::min(ctx->ws[SHZ_WS_RQ_KEY].cap, ctx->ws[SHZ_WS_RQ_T1].cap);
  if (have > 64) cap = std::max(cap, (have - 64) / 4);
  for (int attempt = 0;; ++attempt) {
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RQ_KEY, cap * 4 + 64, &d_key));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RQ_T1, cap * 4 + 64, &d_t1));
    uint64_t count = 0;
    const int32_t rc = shz_fingerprint_batch(ctx, pcm, clip_off, n_clips, fs, amp_min, fan_value,
                                             (flags & SHZ_PCM_DEVICE) | SHZ_OUT_DEVICE, (uint32_t*)d_key, (uint32_t*)d_t1,
                                             hash_off, cap, &count);
    if (rc == SHZ_E_CAPACITY && attempt < 2 && count > cap) {
      // twice what the pass counted: the per-clip fp64 splice parks a redone clip's entries behind the batch's before it
      // moves them into place, so one repeat is enough whichever clips are redone (a second one is the safety net)
      cap = 2 * count + 4096;
      continue;
    }
    if (rc == SHZ_E_CAPACITY) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the extraction needs %llu entries after it was given %llu", who, (unsigned long long)count, (unsigned long long)cap);
    SHZ_TRY(rc);
    break;
  }
  *d_key_out = (const uint32_t*)d_key;
  *d_t1_out = (const uint32_t*)d_t1;
  return SHZ_OK;
}

extern "C" int32_t shz_recognize_batch(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                       const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min,
                                       uint32_t fan_value, uint32_t topn, uint32_t flags, uint32_t* out_sid, int32_t* out_delta,
                                       uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                       uint64_t* out_npairs, float* ms_extract, float* ms_match) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (ms_extract) *ms_extract = 0.f;
  if (ms_match) *ms_match = 0.f;
  // everything that can be refused is refused before the first launch
  if (flags & ~(SHZ_PCM_DEVICE | SHZ_MATCH_FULL_SORT)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_recognize_batch: flags may hold SHZ_PCM_DEVICE and SHZ_MATCH_FULL_SORT");
  if (n_queries == 0) {
    if (n_clips) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_recognize_batch: %u clips belong to no query", n_clips);
    return SHZ_OK;
  }
  SHZ_TRY(shz_check_clip0(ctx, "query_clip0", "query", query_clip0, n_queries, n_clips));
  SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  if (!out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_recognize_batch: NULL buffer");
  SHZ_TRY(shz_match_ready(ctx, t, topn));
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const bool timed = ms_extract || ms_match;
  if (timed) {
    for (hipEvent_t& e : ctx->rq_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->rq_ev[0], ctx->stream));
  }
  // 1) extraction into the library's own buffers
  uint64_t max_frames = 1;
  for (uint32_t c = 0; c < n_clips; ++c)
    max_frames = std::max<uint64_t>(max_frames, shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop));
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0), query_off((size_t)n_queries + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(shz_extract_owned(ctx, "shz_recognize_batch", pcm, clip_off, n_clips, fs, amp_min, fan_value, flags & SHZ_PCM_DEVICE,
                            hash_off.data(), &d_key, &d_t1));
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rq_ev[1], ctx->stream));
  // 2) the match on those buffers
  for (uint32_t q = 0; q <= n_queries; ++q) query_off[q] = hash_off[query_clip0[q]];
  SHZ_TRY(shz_match_device(ctx, t, d_key, d_t1, query_off.data(), n_queries, topn,
                           flags & SHZ_MATCH_FULL_SORT, (int64_t)max_frames - 1, out_sid, out_delta, out_aligned, out_dedup, out_nres,
                           out_nhash, out_npairs));
  if (timed) {
    SHZ_HIP(ctx, hipEventRecord(ctx->rq_ev[2], ctx->stream));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->rq_ev[2]));
    if (ms_extract) SHZ_HIP(ctx, hipEventElapsedTime(ms_extract, ctx->rq_ev[0], ctx->rq_ev[1]));
    if (ms_match) SHZ_HIP(ctx, hipEventElapsedTime(ms_match, ctx->rq_ev[1], ctx->rq_ev[2]));
  }
  return SHZ_OK;
}

// entries the first extraction pass of shz_recognize_batch gets room for (no GPU, no ctx; tests build an input beyond it)
extern "C" uint64_t shz_recognize_estimate(uint64_t frames, uint32_t fan_value) {
  return frames * 12 * (fan_value > 1 ? fan_value - 1 : 1) + 4096;
}
