"""CPU: shz_listener_window (no GPU, no context) -- the window arithmetic of a device-resident listener -- against the
numpy form StreamRecognizer.push uses: H = min over the channels' settled horizons, w0 = max(0, H - window_frames)."""
import numpy as np
import pytest

from shazam_amd import _ffi


def test_window_matches_numpy_form():
    rng = np.random.default_rng(5)
    for channels in (1, 2, 3, 8):
        for window_frames in (0, 1, 21, 107, 1 << 19):
            for _ in range(50):
                settled = rng.integers(0, 400, channels).astype(np.uint64)
                H = int(min(settled.tolist()))
                assert _ffi.listener_window(settled, window_frames) == (H, max(0, H - window_frames))
    big = np.array([(1 << 31) - 1, (1 << 31) - 5], np.uint64)
    assert _ffi.listener_window(big, 107) == ((1 << 31) - 5, (1 << 31) - 5 - 107)
    assert _ffi.listener_window(np.zeros(4, np.uint64), 107) == (0, 0)


def test_window_refuses_no_channels():
    with pytest.raises(_ffi.ShzError) as e:
        _ffi.listener_window(np.zeros(0, np.uint64), 10)
    assert e.value.code == _ffi.E_INVALID


def test_recognize_estimate_needs_no_gpu():
    assert _ffi.recognize_estimate(0, 5) == 4096
    assert _ffi.recognize_estimate(106, 5) == 106 * 12 * 4 + 4096
    assert _ffi.recognize_estimate(10, 1) == 10 * 12 + 4096
