"""The audio of the end-to-end test of the wav.scp -> x-vector route (tests/test_gpu_wav_direct.py) and what must become of it;
tests/test_wav_direct_cpu.py confirms the voiced counts these constructions are chosen for with tests/mfcc_ref.py."""
import numpy as np

FS = 8000
MIN_CHUNK = 25


def waves():
    """(key, rate, int16 wave): "loud" is uniform noise of amplitude 3000, "quiet" of amplitude 3 (well under the energy VAD's
    threshold next to any loud stretch, and under its absolute floor of 5.5 on its own)."""
    rng = np.random.default_rng(2026)

    def loud(sec, fs=FS):
        return rng.integers(-3000, 3001, int(round(sec * fs))).astype(np.int16)

    def quiet(sec):
        return rng.integers(-3, 4, int(round(sec * FS))).astype(np.int16)
    return [("loud-1s", FS, loud(1.0)),
            ("loud-2.5s", FS, loud(2.5)),
            ("loud-4s", FS, loud(4.0)),
            ("half-3s", FS, np.concatenate([loud(1.5), quiet(1.5)])),
            ("quiet-2s", FS, quiet(2.0)),                                  # no voiced frame: dropped ("No voiced frames")
            ("blip-2.2s", FS, np.concatenate([loud(0.2), quiet(2.0)])),    # < MIN_CHUNK voiced frames: rejected ("Minimum chunk size")
            ("wide-2s", 16000, loud(2.0, 16000))]                          # needs --allow-downsample


EXPECTED_KEYS = ["loud-1s", "loud-2.5s", "loud-4s", "half-3s", "wide-2s"]
