"""The four CTC workspace size functions against their formulas (size calls only: no GPU work).

Each function and the entry point that carves the workspace read one layout struct (CtcWs, BeamWs, AlignWs); the
formulas below are written out independently of them.  Negative arguments of cfm_ctc_ws_bytes wrap as size_t
arithmetic does (the function has no early return), hence the mask."""
from nn_conformer_for_speech_recognition_amd import _lib as L

U64 = (1 << 64) - 1
SIZES = (-3, -1, 0, 1, 2, 3, 7, 37, 511)


def test_loss_ws_bytes():
    for B in SIZES:
        for T in SIZES:
            for Smax in SIZES:
                bt = B * T
                want = 4 * (bt + 3 * bt * (2 * Smax + 1) + B) + 8 * B * Smax + 8 * B
                assert L.size_call("cfm_ctc_ws_bytes", B, T, Smax) == want & U64, (B, T, Smax)


def test_beam_ws_bytes():
    for B in SIZES:
        for T in SIZES:
            for W in (-1, 0, 1, 2, 16, 128):
                bt = B * T
                want = 0 if min(B, T, W) <= 0 else 4 * (bt * (2 + 2 * (W + 1)) + B * W)
                assert L.size_call("cfm_ctc_beam_ws_bytes", B, T, W) == want, (B, T, W)


def test_beam_lm_ws_bytes():
    for B in SIZES:
        for T in SIZES:
            for W in (-1, 0, 1, 16, 128):
                for K in (-1, 0, 1, 7, 17, 768):
                    bt = B * T
                    want = 0 if min(B, T, W, K) <= 0 else 4 * (bt * (2 + 2 * K) + 2 * B * W)
                    assert L.size_call("cfm_ctc_beam_lm_ws_bytes", B, T, W, K) == want, (B, T, W, K)


def test_align_ws_bytes():
    for B in SIZES:
        for T in SIZES:
            for Smax in SIZES:
                bt = B * T
                want = 0 if B <= 0 or T <= 0 or Smax < 0 else (5 * bt * (2 * Smax + 1) + 4 * B + 15) & ~15
                assert L.size_call("cfm_ctc_align_ws_bytes", B, T, Smax) == want, (B, T, Smax)


def test_realistic_sizes_do_not_wrap():
    """A training-sized shape and a large one with the longest targets the entry points take."""
    for B, T, Smax in ((32, 373, 120), (256, 4096, 511)):
        bt = B * T
        assert L.size_call("cfm_ctc_ws_bytes", B, T, Smax) == 4 * (bt + 3 * bt * (2 * Smax + 1) + B) + 8 * B * Smax + 8 * B
        assert L.size_call("cfm_ctc_align_ws_bytes", B, T, Smax) == (5 * bt * (2 * Smax + 1) + 4 * B + 15) & ~15
