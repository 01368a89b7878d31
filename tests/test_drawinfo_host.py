"""The debug overlay on the host (no GPU): the sequential definition tests/_drawinfo.py pinned to the reference CLI's -drawinfoN on
geometries whose dimensions are multiples of the block size (elsewhere the reference's dots leave the luma plane, which the definition
deliberately does not follow), the hashes of tests/golden/drawinfo.json, and dsv1_packet_blockinfo's refusals."""
import ctypes as C
import hashlib
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _cabi as A
import _drawinfo as DI
import _drawinfo_cases as K


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("digital-subband-video-1_amd")


def cli_decode(td, mode):
    out = os.path.join(td, "dec%d.yuv" % mode)
    cmd = [A.REF_CLI, "d", "-y", "-inp_" + os.path.join(td, "out.dsv"), "-out_" + out] + (["-drawinfo%d" % mode] if mode else [])
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return np.fromfile(out, dtype=np.uint8)


@pytest.fixture(scope="module")
def ref_runs():
    """per stream fixture: the reference CLI's stream, its plain decode and its -drawinfo1 .. 7 decodes, made once"""
    if not os.path.exists(A.REF_CLI):
        pytest.skip("oracle/_ref binaries were not built")
    runs = {}
    for name, (w, h, seed) in K.STREAMS.items():
        with tempfile.TemporaryDirectory() as td:
            stream = A.ref_cli_encode(K.stream_clip(name), w, h, A.FMT_CLI[A.SUBSAMP_420], K.CLI, td)
            runs[name] = (stream, [cli_decode(td, m).reshape(K.FRAMES, -1) for m in range(8)])
    return runs


@pytest.mark.parametrize("name", list(K.STREAMS))
def test_definition_equals_the_reference_cli(pkg, ref_runs, name):
    w, h, _ = K.STREAMS[name]
    stream, dec = ref_runs[name]
    assert (DI.block_size(w), DI.block_size(h)) == pkg.packet_blockinfo(K.picture_packets(stream)[0], w, h)[:2]
    assert w % DI.block_size(w) == 0 and h % DI.block_size(h) == 0
    for mode in range(1, 8):
        want = dec[mode]
        A.assert_same("%s -drawinfo%d chroma" % (name, mode), want[:, w * h:], dec[0][:, w * h:])
        got = K.define(pkg, stream, dec[0], w, h, mode)
        for t in range(K.FRAMES):
            A.assert_same("%s -drawinfo%d picture %d" % (name, mode, t), got[t, :w * h], want[t, :w * h], shape=(h, w))
    assert hashlib.sha256(dec[7].tobytes()).hexdigest() == K.goldens()[name], "tests/golden/drawinfo.json is stale (tools/make_drawinfo_goldens.py)"


@pytest.mark.parametrize("name", list(K.STREAMS))
def test_fixtures_show_every_kind_of_mark(pkg, ref_runs, name):
    """every P picture has an inter block with a non-zero vector, an intra block and a stable block; 352x288 a partial submask"""
    w, h, _ = K.STREAMS[name]
    pics = K.picture_packets(ref_runs[name][0])
    partial = nP = 0
    for t, p in enumerate(pics):
        bw, bh, has_ref, info = pkg.packet_blockinfo(p, w, h)
        if not has_ref:
            continue
        nP += 1
        inter, intra = info[info["mode"] == 0], info[info["mode"] == 1]
        assert ((inter["mvx"] != 0) | (inter["mvy"] != 0)).any(), "picture %d: no moving inter block" % t
        assert intra.size, "picture %d: no intra block" % t
        assert (info["stable"] & 1).any(), "picture %d: no stable block" % t
        partial += int(((intra["submask"] != 0xF)).sum())
    assert nP >= 3, "too few P pictures for an overlay that leaked into a reference to show"
    if name == "352x288":
        assert partial, "no intra block with a partial submask"


def test_packet_blockinfo_arguments(pkg):
    w, h = 96, 64
    stream, _ = A.orc_encode(K.stream_clip("96x64", frames=2), A.orc_cfg(w, h, A.SUBSAMP_420, **K.KW))
    pk = A.split_packets(stream)
    pics = K.picture_packets(stream)
    bw, bh, has_ref, info = pkg.packet_blockinfo(pics[0], w, h)
    assert (bw, bh, has_ref) == (16, 16, 0) and info.size == 24
    assert not info["mode"].any() and not info["mvx"].any() and not info["submask"].any()        # an I picture: `stable` only
    bw, bh, has_ref, info = pkg.packet_blockinfo(pics[1], w, h)
    assert (bw, bh, has_ref) == (16, 16, 1) and info.size == 24
    L = pkg.lib()
    tab = np.zeros(24, dtype=pkg.BLOCKINFO_DTYPE)
    ints = [C.c_int(0) for _ in range(3)]

    def call(data, n):
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        return L.dsv1_packet_blockinfo(a.ctypes.data, a.size, w, h, C.byref(ints[0]), C.byref(ints[1]), C.byref(ints[2]), tab.ctypes.data, n)

    assert call(pics[1], 24) == 0
    assert call(pics[1], 23) == -2                                   # too small an n
    assert call(pics[1][:len(pics[1]) // 2], 24) == -2               # truncated
    assert call(pics[1][:20], 24) == -2
    assert call(pk[0], 24) == -2 and not (pk[0][5] & 4)              # the metadata packet
    assert call(b"DSVX" + pics[1][4:], 24) == -2
    with pytest.raises(ValueError):
        pkg.packet_blockinfo(pics[1], w, h, n=3)
