"""CPU: the half-pel clips of tests/halfpel_cases.py do what they are for -- the oracle encoder picks vectors with every
(horizontal, vertical) half-pel phase, for luma and for chroma -- and the oracle is pinned to the reference CLI on them
(where oracle/_ref is absent: to the reference's answers in tests/golden/ref_answers.json), so the GPU parity test in test_gpu_halfpel.py stands on the reference itself."""
import tempfile

import numpy as np
import pytest

import _cabi as A
import halfpel_cases as H


@pytest.mark.parametrize("case", range(len(H.CASES)))
def test_clips_cover_every_phase(case):
    w, h, fmt, seed, cli = H.CASES[case]
    clip = H.halfpel_clip(w, h, fmt, seed)
    lum, chrm, intra = H.oracle_phases(clip, w, h, fmt, **cli)
    assert (lum > 0).all(), "luma phases [yh][xh] %s" % lum.tolist()
    assert (chrm > 0).all(), "chroma phases [yh][xh] %s" % chrm.tolist()
    assert intra < lum.sum() // 10


@pytest.mark.parametrize("case", range(len(H.CASES)))
def test_oracle_matches_ref_cli_on_halfpel_clips(case):
    w, h, fmt, seed, cli = H.CASES[case]
    key = "halfpel_%d" % case
    clip = H.halfpel_clip(w, h, fmt, seed)
    flags = ["-gop%d" % cli["gop"], "-qp%d" % cli["qp"], "-rc_mode%d" % cli["rc_mode_cli"], "-scd%d" % cli["scd"]]
    with tempfile.TemporaryDirectory() as td:
        want = A.ref_cli_encode(clip, w, h, A.FMT_CLI[fmt], flags, td) if A.have_ref() else None
        got, recs = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **cli), want_recon=True)
        A.check_ref(key + "/dsv", want, got)
        dec_ref = A.ref_cli_decode(want, td).reshape(clip.shape[0], -1) if want is not None else [None] * clip.shape[0]
        for t in range(clip.shape[0]):
            A.check_ref("%s/decoded%d" % (key, t), dec_ref[t], recs[t], "reference decode != oracle reconstruction at frame %d" % t)
