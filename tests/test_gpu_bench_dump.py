"""GPU: a plain bench.py run prints the headline line of exactly --steps timed steps and nothing of --full, and what
--dump-outputs writes is the last timed step's output: the hashes of the sampled clips equal the oracle's fingerprint of
the same synthetic clips, and hash_off holds every clip's count."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(tmp_path):
    from oracle import cpu_ref as O, synth
    clips, seconds = 6, 4.0
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--clips", str(clips), "--seconds", str(seconds), "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "audio_seconds_fingerprinted_per_second" and line["unit"] == "audio-s/s"
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["roofline"]["kernel_ms_per_step"]["stft_psd"] > 0
    assert not {"cpu_baseline", "extract_stats", "match", "single_query", "match_1M", "db_build_scaling"} & set(line)

    got = {n: np.load(out / f"{n}.npy") for n in ("hash_off", "sample_clips", "key32", "t1")}
    assert all(a.dtype == np.float64 for a in got.values())
    ho, sample = got["hash_off"].astype(np.int64), got["sample_clips"].astype(np.int64)
    assert len(ho) == clips + 1 and ho[0] == 0 and list(sample) == list(range(clips))
    n = int(round(seconds * 44100))
    pos = 0
    for c in sample:
        ok, ot1, _, _ = O.fingerprint_keys(synth.synth_clip(1234, int(c), n, 0, 8000))
        cnt = int(ho[c + 1] - ho[c])
        assert cnt == len(ok) > 0, c
        assert np.array_equal(got["key32"][pos:pos + cnt], ok) and np.array_equal(got["t1"][pos:pos + cnt], ot1), c
        pos += cnt
    assert pos == len(got["key32"]) == len(got["t1"])
