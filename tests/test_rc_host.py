"""The average-bitrate rate control as the C session layer compiles it (include/dsvg_rc.h through dsv1_rc_pick / dsv1_rc_after /
dsv1_rc_seg_bits / dsv1_rc_packet_len, and the host instantiation of dsvg_job_set_quant through dsv1_rc_job_tables; no device) against
tests/rc_model.py, the restatement from the reference's side.  The host's own check -- it refuses a batch whose quantisers differ from
the device's -- compares two compiles of this header and cannot see an error in it; this file can."""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import rc_model as M

N_DRAWS = 200000
SEED = 0x5C0DE


@pytest.fixture(scope="module")
def lib():
    if not __import__("os").path.exists(A.PROD_SO):
        import __graft_entry__ as g
        g.build()
    return A.load_prod_rc()


@pytest.fixture(scope="module")
def reached():
    return set()


def test_random_states_model_against_header(lib, reached):
    """pick, then after on the state pick left (one picture of a stream): the quantiser and all sixteen words, 200 000 times"""
    r = M.rng(SEED)
    cases, dropped = [], 0
    for _ in range(N_DRAWS):
        st, isP, fi, pkt = M.draw_case(r)
        fq, s1, l1 = M.pick(st, isP, fi)
        s2, l2 = M.after(s1, isP, pkt)
        if s2.overflow:                        # undefined in C: compared nowhere
            dropped += 1
            continue
        cases.append((st.words(), isP, fi, pkt, fq, s1.words(), s2.words()))
        reached.update("pick." + x for x in l1)
        reached.update("after." + x for x in l2)
    assert dropped < N_DRAWS * 5 // 100, "%d of %d draws overflow" % (dropped, N_DRAWS)
    n = len(cases)
    buf = np.array([c[0] for c in cases], dtype=np.uint32)
    want1 = np.array([c[5] for c in cases], dtype=np.uint32)
    want2 = np.array([c[6] for c in cases], dtype=np.uint32)
    wantq = np.array([c[4] for c in cases], dtype=np.int64)
    gotq = np.empty(n, dtype=np.int64)
    got1 = np.empty_like(buf)
    base = buf.ctypes.data
    for i, c in enumerate(cases):
        gotq[i] = lib.dsv1_rc_pick(base + 64 * i, c[1], c[2])
    got1[...] = buf
    for i, c in enumerate(cases):
        lib.dsv1_rc_after(base + 64 * i, c[1], c[3])
    bad = np.nonzero((gotq != wantq) | (got1 != want1).any(axis=1) | (buf != want2).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        c = cases[i]
        raise AssertionError("%d of %d cases differ; first: state %s isP %d forced %d pkt %d\n quant %d want %d\n pick  %s\n want  %s\n after %s\n want  %s" % (
            bad.size, n, dict(zip(M.FIELDS, c[0])), c[1], c[2], c[3], gotq[i], wantq[i], got1[i].tolist(), c[5], buf[i].tolist(), c[6]))


def test_generator_alone_stays_defined():
    """the generator's own share of overflow cases, on another seed, and that it never draws a state the model refuses"""
    r = M.rng(SEED + 1)
    dropped = 0
    for _ in range(20000):
        st, isP, fi, pkt = M.draw_case(r)
        fq, s1, _ = M.pick(st, isP, fi)            # raises ValueError for a refused state
        s2, _ = M.after(s1, isP, pkt)
        dropped += s2.overflow
        assert 5 <= fq <= M.MAXQ or s2.overflow
    assert dropped < 20000 * 5 // 100


def test_model_flags_overflow_and_refuses_division_by_zero():
    big = M.make_state(bitrate=60000000, fps_num=1, fps_den=8, bpf_avg=1 << 30, rc_quant=1000)
    assert M.pick(big, 1, 0)[1].overflow           # abs(bpf - need) << 9 leaves int32
    assert M.pick(M.make_state(fps_num=1 << 27), 1, 0)[1].overflow           # fps_num << 5
    for bad in (M.make_state(bitrate=0), M.make_state(fps_den=0), M.make_state(fps_den=-1)):
        with pytest.raises(ValueError):
            M.pick(bad, 0, 0)
    with pytest.raises(ValueError):
        M.after(M.make_state(bpf_reset=0xFFFFFFFF, bitrate=100000), 0, 10)


def test_seg_bits(lib):
    got = np.array([lib.dsv1_rc_seg_bits(v) for v in range(-70000, 70001)])
    want = np.array([M.seg_bits(v) for v in range(-70000, 70001)])
    A.assert_same("seg_bits over [-70000, 70000]", got, want)


def test_packet_len(lib, reached):
    r = M.rng(SEED + 2)
    fixed = [(14, [0, 0, 0], [0, 0, 0]), (100, [14, -15, 254], [8, 9, 7]), (100, [-255, 15, -14], [16, 1, 0]), (0, [-70000, 70000, 1], [0xFFFFFFF0, 0x7FFFFFFF, 1 << 20])]
    for prefix, dc, bits in fixed + [M.draw_packet(r) for _ in range(20000)]:
        want, labels = M.packet_len(prefix, dc, bits)
        got = lib.dsv1_rc_packet_len(prefix, (C.c_int * 3)(*dc), (C.c_ulonglong * 3)(*bits))
        assert got == want, (prefix, dc, bits, got, want)
        reached.update("packet." + x for x in labels)


def test_job_tables(lib):
    out = (C.c_int * 76)()
    got, want = [], []
    for isP in (0, 1):
        for q in range(5, M.MAXQ + 1):
            lib.dsv1_rc_job_tables(q, isP, out)
            got.append(list(out))
            want.append(M.job_table_words(q, isP))
    A.assert_same("job tables for quant 5..2047, I and P", np.array(got), np.array(want), shape=(2 * (M.MAXQ - 4), 76))


def test_every_label_reached(reached):
    """runs after the tests above (file order): their inputs together went through every branch the model names"""
    assert reached == M.ALL_LABELS, "not reached: %s; unknown: %s" % (sorted(M.ALL_LABELS - reached), sorted(reached - M.ALL_LABELS))
