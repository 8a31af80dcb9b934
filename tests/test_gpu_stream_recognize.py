"""GPU: StreamRecognizer -- stereo listeners pushed in the reference's 8192-sample chunks (recognizer.py:21-25, 357-392)
recognise what they hear from the settled hashes of a sliding window, in one batched match per push.  After every push
each listener's results equal db.match on the same window cut from the whole-signal fingerprint; for two listeners
also the oracle's align_matches over a DictDB."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192
HOP = 2048


def test_stereo_listeners_window_results():
    import shazam_amd as S
    from oracle import cpu_ref as O, synth
    from shazam_amd import harness
    ctx = S.get_context(0)
    n_songs, song_len = 50, 44100 * 20
    songs = [synth.music_clip(31, i, song_len) for i in range(n_songs)]
    db, odb = S.get_database("hip")(ctx=ctx), O.DictDB()
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    for i in range(n_songs):
        sid = db.insert_song(f"song{i}", f"{i:040x}", int(len(set(zip(k[ho[i]:ho[i + 1]].tolist(), t1[ho[i]:ho[i + 1]].tolist())))))
        db.set_song_fingerprinted(sid)
    db.insert_clips(k, t1, ho, 1)
    db.finalize()
    for i in range(n_songs):   # the oracle's table holds the rows (hex hashes) of the two songs its listeners hear
        hs = set(zip(S.hex_of_keys(ctx, k[ho[i]:ho[i + 1]]), t1[ho[i]:ho[i + 1]].tolist())) if i in (3, 17) else set()
        osid = odb.insert_song(f"song{i}", f"{i:040x}", max(1, len(hs)))
        assert osid == i + 1
        odb.insert_hashes(osid, hs)
    rng = np.random.default_rng(8)
    picks = [3, 17, 5, 9, 22, 30, 41, 48]
    starts = [int(rng.integers(1, 200)) * HOP + int(rng.integers(1, HOP)) for _ in picks]   # not hop-aligned
    length = 44100 * 8
    listeners = []
    for j, (s, a) in enumerate(zip(picks, starts)):
        clean = songs[s][a:a + length]
        left = harness.mix(clean, synth.traffic_noise(70, 2 * j, length), 10)
        right = harness.mix(clean, synth.traffic_noise(70, 2 * j + 1, length), 10)
        listeners.append((left, right))
    n = len(listeners)
    rec = S.StreamRecognizer(db, n, channels=2, window_seconds=5, topn=3)
    whole = [[ctx.fingerprint_batch(ch, np.array([0, length], np.uint64))[:2] for ch in L] for L in listeners]
    seen_ok = [False] * n
    for p, a in enumerate(range(0, length, CHUNK)):
        ending = a + CHUNK >= length
        out = rec.push([[L[0][a:a + CHUNK], L[1][a:a + CHUNK]] for L in listeners], end=True if ending else None)
        assert len(out) == n
        for l in range(n):
            res, w0 = out[l]
            H = min(rec.fp.state(2 * l + c)["settled"] for c in range(2))
            assert w0 == max(0, H - rec.window_frames)
            keys, qo = [], []
            for c in range(2):
                e = rec.fp.state(2 * l + c)["emitted"]
                wk, wt = whole[l][c]
                wk, wt = wk[:e], wt[:e]          # what the stream has emitted: a prefix of the whole fingerprint
                sel = wt >= w0
                keys.append(wk[sel])
                qo.append((wt[sel] - w0).astype(np.uint32))
            kk, qq = np.concatenate(keys), np.concatenate(qo)
            if len(kk) == 0:
                assert res == []
                continue
            r = db.match(kk, qq, np.array([0, len(kk)], np.uint64), 3)
            want = S._result_dicts(db, r, 0, int(r["nhash"][0]))
            assert res == want, (p, l)
            if l < 2 and (p % 8 == 7 or ending):
                hs = set(zip(S.hex_of_keys(ctx, kk), qq.tolist()))
                matches, dedup = O.return_matches(hs, odb)
                ow = O.align_matches(matches, dedup, len(hs), odb, topn=3)
                assert [(d["song_id"], d["offset"], d["hashes_matched_in_input"], d["input_total_hashes"]) for d in res[:1]] == \
                       [(d["song_id"], d["offset"], d["hashes_matched_in_input"], d["input_total_hashes"]) for d in ow[:1]], (p, l)
            if a + CHUNK >= 44100 * 5:
                start_frame = starts[l] // HOP
                top = res[0]
                assert top["song_id"] == picks[l] + 1, (p, l, top)
                # the window is a clip recorded from stream frame w0 = song frame start_frame + w0
                assert abs(top["offset"] - (start_frame + w0)) <= 1, (p, l, top["offset"], start_frame, w0)
                seen_ok[l] = True
    assert all(seen_ok)
    rec.close()
    db.close()
