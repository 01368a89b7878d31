"""Every branch of the device-resident rate control (k_rc.hip: include/dsvg_rc.h and dsvg_job_set_quant as the device compiles them,
the indexing by d0 / slot / next) on built states, against tests/rc_model.py -- the restatement from the reference's side that
tests/test_rc_ref.py pins to the reference library itself.

Operator part: dsvg_op_rc builds job records from plain arrays, makes ONE launch_rc and returns everything the kernel may touch.  No
pictures.  Whatever lies outside the launched range, belongs to a skipped job (slot < 0) or to an unused slot must come back as it
went in: poison or input bytes.

Session part (below): every seeded case of tests/rc_cases.py RC_SEEDS through the product's three session paths."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import _cabi as A
import rc_cases as RC
import rc_model as M
from test_rc_ref import FMT, case_clip, case_encoder, case_orc, pictures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = A.load_prod_rc()
    assert L.dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return L


@pytest.fixture(scope="module")
def launches():
    return RC.op_launches()


def run_launch(L, la):
    jobs = (A.OpRcJob * la.n)()
    for j, jb in enumerate(la.jobs):
        o = jobs[j]
        o.isP, o.forced_intra, o.prefix_len, o.slot, o.next, o.quant = jb["isP"], jb["forced_intra"], jb["prefix_len"], jb["slot"], jb["next"], jb["quant"]
        o.dc[:] = jb["dc"]
        o.total_bits[:] = jb["total_bits"]
    states = A.rc_state_words(la.states)
    before = states.copy()
    out = (A.OpRcOut * la.n)()
    A.chk(L, L.dsvg_op_rc(la.n, jobs, la.nslots, states.ctypes.data, la.d0, la.count, la.mode, out))
    got = np.frombuffer(out, dtype=np.int32).reshape(la.n, 80)
    return before, states, got[:, 0], got[:, 1:77], got[:, 77:80]


def check_launch(L, la):
    before, states, quant, tables, rc = run_launch(L, la)
    what = "count %d d0 %d mode %d" % (la.count, la.d0, la.mode)
    A.assert_same(what + ": states", states, A.rc_state_words(la.want_states), shape=(la.nslots, 16))
    A.assert_same(what + ": quant", quant, np.array(la.want_quant, dtype=np.int64).astype(np.int32))
    A.assert_same(what + ": tables", tables, np.array(la.want_tables, dtype=np.int64).astype(np.int32), shape=(la.n, 76))
    A.assert_same(what + ": plane-sum rc words", rc, np.array(la.want_rc, dtype=np.int64).astype(np.int32), shape=(la.n, 3))
    # the same once more, said directly: nothing outside the launch's reach moved
    used = {jb["slot"] for jb in la.jobs[la.d0:la.d0 + la.count] if jb["slot"] >= 0}
    idle = [s for s in range(la.nslots) if s not in used]
    assert np.array_equal(states[idle], before[idle]), what + ": a state no launched job owns changed"
    written = set()
    for j in range(la.d0, la.d0 + la.count):
        jb = la.jobs[j]
        if jb["slot"] >= 0:
            written.add(j if la.mode == 0 else jb["next"])
    for j in range(la.n):
        if j not in written:
            assert quant[j] == np.int32(la.jobs[j]["quant"]) and (tables[j] == A.OP_RC_POISON).all(), what + ": job %d's tables were written" % j
        live = la.mode == 1 and la.d0 <= j < la.d0 + la.count and la.jobs[j]["slot"] >= 0
        if not live:
            assert (rc[j] == A.OP_RC_POISON).all(), what + ": job %d's plane sums were written" % j


@pytest.mark.parametrize("case", range(len(RC.OP_LAUNCHES)), ids=["count%d-d0_%d-mode%d" % c for c in RC.OP_LAUNCHES])
def test_one_launch_against_the_model(lib, launches, case):
    check_launch(lib, launches[case])


def test_launches_reach_every_label(launches):
    reached = set().union(*[la.labels for la in launches])
    assert reached == M.ALL_LABELS, "not reached: %s" % sorted(M.ALL_LABELS - reached)
    la = launches
    assert any(jb["slot"] < 0 for x in la for jb in x.jobs[x.d0:x.d0 + x.count])
    assert any(jb["next"] < 0 and jb["slot"] >= 0 for x in la if x.mode == 1 for jb in x.jobs[x.d0:x.d0 + x.count])
    assert any(jb["next"] >= x.d0 + x.count for x in la if x.mode == 1 for jb in x.jobs[x.d0:x.d0 + x.count])
    assert any(0 <= jb["next"] < x.d0 for x in la if x.mode == 1 for jb in x.jobs[x.d0:x.d0 + x.count])
    assert any(jb["next"] >= 0 and x.jobs[jb["next"]]["isP"] != jb["isP"] for x in la if x.mode == 1 for jb in x.jobs[x.d0:x.d0 + x.count])


def test_every_frame_quantiser_through_the_device_tables(lib):
    """the device instantiation of dsvg_job_set_quant (dsvg_lb2u's loop, the level quantisers, the chroma limit) over its whole
    domain: one launch, a job per quantiser 5..2047 and picture type"""
    check_launch(lib, RC.QuantDomainLaunch())


def test_operator_refuses_what_would_index_outside(lib):
    la = RC.OpLaunch(1, 4, 0, 1)
    jobs = (A.OpRcJob * la.n)()
    states = A.rc_state_words(la.states)
    out = (A.OpRcOut * la.n)()
    for field, value, d0, count in (("slot", la.nslots, 0, 4), ("next", la.n, 0, 4), ("next", -2, 0, 4), ("slot", 0, la.n - 1, 2), ("slot", 0, -1, 2)):
        C.memset(jobs, 0, C.sizeof(jobs))
        for j in range(la.n):
            jobs[j].slot, jobs[j].next = j, -1
        setattr(jobs[1], field, value)
        assert lib.dsvg_op_rc(la.n, jobs, la.nslots, states.ctypes.data, d0, count, 1, out) != 0


# ---- seeded sessions: every RC_SEEDS case through the product's three session paths ----------------------------------------------------
# The oracle's bytes for these cases are the reference's (tests/test_rc_ref.py).  The encoders are seeded before the first submit --
# the session loads their state into the device then (rc_load, dsv1_enc.c) -- and after the last collect both the device's copy of
# the state (dsvg_rc_download) and the encoder struct must hold what the model says.
@pytest.fixture(scope="module")
def pkg():
    m = importlib.import_module("digital-subband-video-1_amd")
    assert m.lib().dsvg_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return m


def _group_key(case):
    return (tuple(sorted(case["cli"].items())), RC.cfg_fields(case)[1], case["frames"], case["F"], case["calls"])


def session_groups():
    """cases that can share a batch (one configuration, frame rate and call layout), as lists of names"""
    groups = {}
    for c in RC.RC_SEEDS:
        groups.setdefault(_group_key(c), []).append(c["name"])
    return list(groups.values())


GROUPS = session_groups()


@pytest.fixture(scope="module")
def expected():
    """per case: the oracle's stream without the end-of-stream packet, and the model's final state over it"""
    out = {}
    for c in RC.RC_SEEDS:
        data, _ = case_orc(c, eos=False)
        out[c["name"]] = (data, RC.replay(c, pictures(data))[2])
    return out


def _apply(enc, fields):
    for k, v in fields.items():
        setattr(enc, k, v)


def run_group(pkg, names, serial, pipelined):
    """the group's cases as the streams of one Batch -> ([bytes per stream], device states (S, 16) or None, [struct state words + max_q_step])"""
    cases = [RC.RC_SEEDS[RC.RC_SEED_NAMES.index(n)] for n in names]
    S, F, calls = len(cases), cases[0]["F"], cases[0]["calls"]
    clips = np.stack([case_clip(c) for c in cases])
    old = os.environ.get("DSV1_ABR_SERIAL")
    os.environ["DSV1_ABR_SERIAL"] = "1" if serial else "0"
    try:
        b = pkg.Batch(case_encoder(pkg, dict(cases[0], par={k: v for k, v in cases[0]["par"].items() if k in ("fps_num", "fps_den")})), S, F)
    finally:
        if old is None:
            del os.environ["DSV1_ABR_SERIAL"]
        else:
            os.environ["DSV1_ABR_SERIAL"] = old
    out = [b""] * S
    try:
        for s, c in enumerate(cases):                          # parameters and seed, before the first submit
            e = b.encoder(s)
            _apply(e, RC.cfg_fields(c)[0])
            _apply(e, c["seed"])

        def submit(k):
            for s, c in enumerate(cases):
                assert all(t % F == 0 for t in c["changes"]), "a batch takes parameter changes between submits"
                _apply(b.encoder(s), c["changes"].get(k * F, {}))
            b.submit(np.ascontiguousarray(clips[:, k * F:(k + 1) * F]))

        def collect():
            for s, o in enumerate(b.collect()):
                out[s] += bytes(o)
        if pipelined:                                          # call k + 1 is enqueued before call k is collected
            submit(0)
            for k in range(1, calls):
                submit(k)
                collect()
            collect()
        else:
            for k in range(calls):
                submit(k)
                collect()
        dev = None
        if not serial:
            dev = np.zeros((S, 16), dtype=np.uint32)
            A.chk(b.L, b.L.dsvg_rc_download(C.c_void_p(b.ctx), 0, S, C.c_void_p(dev.ctypes.data)))
        struct = [[int(getattr(b.encoder(s), f)) & 0xFFFFFFFF for f in M.STATE_FIELDS + ("max_q_step",)] for s in range(S)]
    finally:
        b.close()
    return out, dev, struct


def check_group(names, expected, out, dev, struct, what):
    for s, n in enumerate(names):
        want, fin = expected[n]
        assert out[s] == want, "%s: case %s differs from the oracle" % (what, n)
        assert struct[s] == [M.u32(fin[f]) for f in M.STATE_FIELDS + ("max_q_step",)], "%s: case %s: the encoder struct's state" % (what, n)
        if dev is not None:
            A.assert_same("%s: case %s: the device's state" % (what, n), dev[s], np.array(fin.words(), dtype=np.uint32))


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=["+".join(g) for g in GROUPS])
def test_seeded_batch_with_device_rate_control(pkg, expected, group):
    names = GROUPS[group]
    check_group(names, expected, *run_group(pkg, names, serial=False, pipelined=False), what="device rate control")
    if RC.RC_SEEDS[RC.RC_SEED_NAMES.index(names[0])]["calls"] > 1:
        # the renormalisation on the last picture of a call while the next call is already enqueued (wrap_last_of_call), parameter
        # changes behind a call in flight (over_then_under, thresholds)
        check_group(names, expected, *run_group(pkg, names, serial=False, pipelined=True), what="device rate control, two calls in flight")


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=["+".join(g) for g in GROUPS])
def test_seeded_batch_on_the_frame_serial_host_path(pkg, expected, group):
    names = GROUPS[group]
    check_group(names, expected, *run_group(pkg, names, serial=True, pipelined=False), what="DSV1_ABR_SERIAL=1")


@pytest.mark.parametrize("name", RC.RC_SEED_NAMES)
def test_seeded_dsv_enc(pkg, expected, monkeypatch, name):
    """the reference's frame-at-a-time API on the product library, the struct seeded between dsv_enc_start and the first dsv_enc"""
    case = RC.RC_SEEDS[RC.RC_SEED_NAMES.index(name)]
    monkeypatch.setenv("DSV1_ENC_LOOKAHEAD", "12" if case["cli"]["gop"] else "16")
    enc = case_encoder(pkg, case)
    states = []
    got, counts = A.drive_dsv_enc(pkg.lib(), enc, case_clip(case), RC.W, RC.H, FMT, changes=case["changes"], rc_seed=case["seed"],
                                  states_out=states, flush_calls=True)
    want, fin = expected[name]
    assert got[:-14] == want and len(got) == len(want) + 14, "dsv_enc differs from the oracle"       # (+ the end-of-stream packet)
    assert list(states[-1]) == [M.u32(fin[f]) for f in M.STATE_FIELDS], "the encoder struct's state after the last picture"
    assert int(enc.max_q_step) == fin["max_q_step"]
