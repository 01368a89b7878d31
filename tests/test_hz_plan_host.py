"""CPU: the model of the entropy pack stage (tests/hz_plan.py) against the oracle, and the coverage of its labels by the cases of
tests/hz_cases.py -- from the oracle alone, nothing of the product is loaded.

  * the model's plain bit writer reproduces the oracle's plane payload byte for byte on every case of both lists, on the tile
    clips and on the HZ_CASES shapes of tests/test_gpu_ops.py: that pins the bit offsets the labels are derived from;
  * nscan, ll_end and nchunks agree with what the oracle's scan produces (region overlap geometries included);
  * every label that is not declared unreachable is hit by a case, and every case hits each label it is listed for;
  * the round sequence is self-consistent: entries consumed per chunk equal its count, bits summed over rounds the writer's.
"""
import ctypes as C

import numpy as np
import pytest

import _cabi as A
import hz_cases as HC
import hz_plan as H
from test_gpu_ops import HZ_CASES as HZ_SHAPES, stab_for

OP = HC.op_cases()


def payload_of(buf, rec):
    nbytes = (rec["bits"] + 7) // 8
    return bytes(buf[rec["at"]:rec["at"] + nbytes])


def check_plane(model, rec, buf, what):
    """the writer's bytes and the model's sums against the oracle's record of one plane"""
    want = payload_of(buf, rec)
    got, nbits = H.write_plane(rec["entries"].tolist())
    assert nbits == rec["bits"], "%s: the writer makes %d bits, the oracle %d" % (what, nbits, rec["bits"])
    assert got == want, "%s: the writer's payload differs from the oracle's: %s" % (what, model.explain(got, want))
    assert model.total_bits == nbits, what
    # the round sequence: entries and bits per chunk
    bit, per = 0, np.bincount(rec["entries"][:, 0] // H.HZ_CHUNK, minlength=model.nchunks)
    for c in model.chunks:
        assert c.bit_off == bit and sum(r.n for r in c.rounds) == c.nnz == int(per[c.index]), (what, c.index)
        ent = rec["entries"][c.lo:c.hi].tolist()
        prev = rec["entries"][c.lo - 1].tolist() if c.lo else None
        alone = sum(H.len_ueg(p - (q[0] if q else -1) - 1) + (H.len_neg(q[1]) if q else 0) for p, q in zip([e[0] for e in ent], [prev] + ent[:-1]))
        assert c.bits == sum(r.bits for r in c.rounds) == alone, (what, c.index)
        bit += c.bits
    assert model.labels <= set(H.LABELS), model.labels - set(H.LABELS)


def scan_counts(w, h):
    """cells the oracle's scan visits: a plane of all-large coefficients makes every cell an entry but cell 0"""
    co = np.full(w * h, 1 << 20, dtype=np.int32)
    pl, _, _, rec = HC.op_plane(w, h, co)
    return rec["entries"]


@pytest.mark.parametrize("w,h", [(8, 8), (16, 16), (20, 30), (36, 20), (100, 52), (250, 130), (360, 200), (180, 100), (352, 240), (64, 64)])
def test_geometry_is_the_oracle_scan(orc, w, h):
    ll_end, nscan, nchunks = H.geometry(w, h)
    e = scan_counts(w, h)
    assert len(e) == nscan - 1 and int(e[-1, 0]) == nscan - 1 and int(e[0, 0]) == 1, "the oracle walks %d cells, the model says %d" % (len(e) + 1, nscan)
    assert ll_end == H.rsu(w, 3) * H.rsu(h, 3) and nchunks == -(-nscan // 2048)
    assert (nscan > w * h) == H.overlaps(w, h), "cells seen twice exactly where the regions overlap"
    # ll_end is where the oracle leaves the LL region: an LL-only plane has no entry at or past it
    co = np.zeros((h, w), dtype=np.int32)
    co[:H.rsu(h, 3), :H.rsu(w, 3)] = 1 << 20
    rec = HC.op_plane(w, h, co.reshape(-1))[3]
    assert len(rec["entries"]) == ll_end - 1 and (ll_end == 1 or int(rec["entries"][-1, 0]) == ll_end - 1)


def test_some_geometry_overlaps():
    assert H.overlaps(36, 20) and H.overlaps(180, 100) and not H.overlaps(128, 128)
    assert H.geometry(360, 200)[0] == 1125 and H.geometry(704, 480)[0] == 5280 and H.geometry(2048, 2080)[1:] == (4259840, 2080)


@pytest.mark.parametrize("name", list(OP))
def test_operator_case(orc, name):
    w, h, co, labels = OP[name]
    model, buf, _, rec = HC.op_plane(w, h, co)
    check_plane(model, rec, buf, name)
    assert set(labels) <= model.labels, "%s is listed for %s" % (name, sorted(set(labels) - model.labels))
    assert not any(c.packed for c in model.chunks)


def pipe_models(name):
    clip, stream, recs, pictures = HC.pipe_oracle(name)
    packets = A.split_packets(stream)
    for t, pic in enumerate(pictures):
        for rec in pic["planes"]:
            yield t, pic, rec, HC.model_of(rec), packets[pic["packet"]]


@pytest.mark.parametrize("name", [c[0] for c in HC.PIPE_CASES])
def test_pipeline_case(orc, name):
    _, g, content, qp, n, labels = HC.pipe_case(name)
    got, kinds = set(), []
    for t, pic, rec, model, packet in pipe_models(name):
        check_plane(model, rec, packet, "%s picture %d plane %d" % (name, t, rec["cur_plane"]))
        assert (rec["w"], rec["h"]) == A.coef_dims(g[0], g[1], g[2], rec["cur_plane"])
        assert all(c.packed == (c.index * 2048 >= model.ll_end) for c in model.chunks)
        got |= model.labels
        kinds.append(pic["kind"])
    assert kinds[::3] == ["I"] + ["P"] * (n - 1), kinds[::3]
    assert set(labels) <= got, "%s is listed for %s" % (name, sorted(set(labels) - got))


def test_pipeline_geometries():
    """what the issue asks of the pipeline geometries"""
    assert all(H.geometry(*A.coef_dims(32, 32, HC.F420, c))[2] == 1 for c in range(3)), "32x32 4:2:0: every plane a single chunk"
    assert H.geometry(360, 200)[0] % 4 and H.overlaps(*A.coef_dims(360, 200, HC.F420, 1))
    assert H.geometry(704, 480)[0] // 2048 == 2, "two whole LL chunks before the straddling one"


def test_scene_cut_case(orc):
    kinds = [[p["kind"] for p in run[3]] for run in HC.cut_oracle()]
    assert kinds == [["I", "P", "P"], ["I", "I", "P"]], "one frame step with an I job and a P job: %s" % kinds
    for n in HC.CUT_NAMES:
        for t, pic, rec, model, packet in pipe_models(n):
            check_plane(model, rec, packet, "%s picture %d plane %d" % (n, t, rec["cur_plane"]))


def test_tile_clips(orc):
    """the three tile labels, from the oracle: clip A's I picture has entries in the second tile of the 256-thread scan and before
    it, clip B's pictures none there, clip A's P picture its first non-empty chunk there"""
    o = HC.tile_oracle()
    assert H.scan_threads(HC.TILE_STREAMS) == 256 and H.scan_threads(32) == 1024
    lab = {}
    for k, (clip, stream, recs, pictures) in o.items():
        packets = A.split_packets(stream)
        assert [p["kind"] for p in pictures] == ["I", "P"]
        for pic in pictures:
            for rec in pic["planes"]:
                model = HC.model_of(rec, njobs=HC.TILE_STREAMS)
                check_plane(model, rec, packets[pic["packet"]], "tile clip %s %s plane %d" % (k, pic["kind"], rec["cur_plane"]))
                assert "sc.256" in model.labels
                if rec["cur_plane"] == 0:
                    assert model.nchunks == 2080
                    lab[k + pic["kind"]] = {l for l in model.labels if l.startswith("sc.tile2")}
                    assert not ({l for l in HC.model_of(rec, njobs=32).labels if l.startswith("sc.tile2")}), "one tile of 8192 chunks with 1024 threads"
                else:
                    assert not any(l.startswith("sc.tile2") for l in model.labels)
    assert lab == {"AI": {"sc.tile2.entries"}, "AP": {"sc.tile2.first"}, "BI": {"sc.tile2.empty"}, "BP": {"sc.tile2.empty"}}, lab


@pytest.mark.parametrize("w,h,cur_plane", HZ_SHAPES)
def test_writer_on_the_operator_shapes(orc, w, h, cur_plane):
    """test_gpu_ops.test_encode_decode_plane's planes, a few seeds: the writer's payload is the oracle's"""
    for seed, isP, q in ((1, 0, 16), (2, 1, 313), (3, 1, 3000)) if w * h < 200000 else ((2, 1, 313),):       # (the large planes: one seed, for the model's time)
        rng = np.random.default_rng(w + 3 * h + seed)
        fw, fh = (w * 2, h * 2) if cur_plane else (w, h)
        st, keep = stab_for(rng, fw, fh, isP, cur_plane)
        co = rng.laplace(0, 40 if q < 1000 else 400, size=(h, w)).astype(np.int32)
        co[: h // 8, : w // 8] *= 16
        co = co.reshape(-1)
        buf = np.zeros(w * h * 8 + 64, dtype=np.uint8)
        bs = A.BS(A.u8p(buf), 0)
        _, recs = HC.recorded(lambda: orc.orc_encode_plane(C.byref(bs), C.byref(A.Coefs(A.i32p(co), w, h)), q, C.byref(st)))
        model = H.Plane(w, h, recs[0]["entries"], "P" if isP else "I", "op", 1)
        assert not len(recs[0]["entries"]) or int(recs[0]["entries"][-1, 0]) < model.nscan
        check_plane(model, recs[0], buf, "%dx%d seed %d" % (w, h, seed))


def test_every_label_is_reached(orc):
    """a condition, not a measurement: no label may be left out"""
    got = set()
    for name, (w, h, co, labels) in OP.items():
        got |= HC.op_plane(w, h, co)[0].labels
    for c in HC.PIPE_CASES:
        for t, pic, rec, model, packet in pipe_models(c[0]):
            got |= model.labels
    for k, (clip, stream, recs, pictures) in HC.tile_oracle().items():
        for pic in pictures:
            got |= HC.model_of(pic["planes"][0], njobs=HC.TILE_STREAMS).labels
    assert set(H.UNREACHABLE) <= set(H.LABELS)
    missing = set(H.LABELS) - set(H.UNREACHABLE) - got
    assert not missing, "no case reaches %s" % sorted(missing)
    assert not (got & set(H.UNREACHABLE)), "declared unreachable, but reached: %s" % sorted(got & set(H.UNREACHABLE))
    # the labels each seam owns are reached THROUGH that seam
    op = set().union(*(HC.op_plane(w, h, co)[0].labels for w, h, co, _ in OP.values()))
    owned = [l for l in H.LABELS if l.startswith(("r64.", "w.", "pl.", "un."))]
    assert set(owned) <= op, sorted(set(owned) - op)


def test_writer_codes():
    """bs.c:129-206 by hand: UEG(0) = '1', UEG(1) = '001', UEG(2) = '011', NEG(1) = '10', NEG(-1) = '11', NEG(2) = '0010'"""
    assert [H.code_ueg(v) for v in (0, 1, 2, 3)] == [(1, 1), (1, 3), (3, 3), (1, 5)]
    assert [H.code_neg(v) for v in (1, -1, 2, -3)] == [(2, 2), (3, 2), (2, 4), (7, 4)]
    assert all(H.code_ueg(v)[1] == H.len_ueg(v) for v in range(70000)) and H.len_neg(-40000) == 2 * 15 + 2
    assert H.write_plane([(5, 3), (6, -1)]) == (bytes([0b01001101, 0b10110000]), 12)     # U(5) | U(0) N(3) | N(-1)
