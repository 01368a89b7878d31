#!/usr/bin/env python3
"""Frames/s of the drop-in decoder (dsv_dec: one picture per call, host sync per picture) on a 1080p GOP=12 stream, and of the
batched decoder.  With --formats: only the cost of the decoder's output formats (dsv1_decbatch_set_output_format) -- time per
dsv1_decbatch_decode call with device output for packed planar (the pass that was there before), NV12 and P010 of 4:2:0 streams and
for packed planar and 4:2:0 NV12 of 4:4:4 streams, the settings alternating run by run; then, in a run of its own, the output
kernels' own time (dsvg_prof_get)."""
import ctypes as C, importlib, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import _cabi as A
pkg = importlib.import_module("digital-subband-video-1_amd")
L = pkg.lib()
W, H, FMT, N = 1920, 1080, A.SUBSAMP_420, 48


def output_formats(S, runs=9, warm=2):
    PIX = pkg.PixFormat
    cases = [(A.SUBSAMP_420, [("packed planar (no format set)", None, A.SUBSAMP_420), ("NV12", PIX(pkg.PIX_SEMIPLANAR_UV), A.SUBSAMP_420),
                              ("P010", PIX(pkg.PIX_SEMIPLANAR_UV, 10, 1), A.SUBSAMP_420)]),
             (A.SUBSAMP_444, [("packed planar 4:4:4 (no format set)", None, A.SUBSAMP_444), ("4:4:4 -> 4:2:0 NV12", PIX(pkg.PIX_SEMIPLANAR_UV), A.SUBSAMP_420)])]
    status = (C.c_int * S)(); fnum = (C.c_uint32 * S)()
    for fmt, settings in cases:
        clip = A.gen_clip(W, H, fmt, 0x10800003, 12, style=0)
        clip = np.concatenate([clip] * (N // 12), axis=0)
        pk = A.split_packets(pkg.encode_clip(clip, W, H, fmt, qp=85, gop=12, rc_mode_cli=1))
        keep = [np.frombuffer(bytes(p) + b"\0" * 16, dtype=np.uint8).copy() for p in pk]
        calls = []
        for k, p in enumerate(pk):
            bufs = (pkg.Buf * S)()
            for s in range(S):
                bufs[s].data = keep[k].ctypes.data_as(C.POINTER(C.c_uint8)); bufs[s].len = len(p)
            calls.append(bufs)
        npic = sum(1 for p in pk if p[5] & 4)
        d = pkg.DecBatch(W, H, fmt, S)
        dst = {}
        for name, pf, osub in settings:
            d.set_output_format(pf, osub)
            dst[name] = (d.dev_alloc(), d.frame_bytes)

        def one_run(name, pf, osub):
            d.set_output_format(pf, osub)
            p, fb = dst[name]
            d.sync()
            t0 = time.perf_counter()
            for bufs in calls:
                rc = L.dsv1_decbatch_decode(d.h, bufs, p, fb, 1, status, fnum)
                assert rc == 0, L.dsvg_last_error()
            d.sync()
            return (time.perf_counter() - t0) / npic * 1e3        # ms per call that decodes pictures

        times = {name: [] for name, _, _ in settings}
        for r in range(warm + runs):                       # the settings alternate run by run: drift hits all of them alike
            for name, pf, osub in settings:
                t = one_run(name, pf, osub)
                if r >= warm:
                    times[name].append(t)
        print("%d streams 1920x1080 subsampling 0x%x GOP 12, device output, %d picture calls per run, %d runs after %d warm-up runs:" % (S, fmt, npic, runs, warm))
        for name, _, _ in settings:
            t = sorted(times[name])
            print("  %-38s %7.3f ms per call (median; min %.3f, max %.3f), %d bytes per frame" % (name, statistics.median(t), t[0], t[-1], dst[name][1]))
        # the output kernels' own time, measured in a run of its own (bracketing a kernel moves it onto the first coding stream)
        nk = L.dsvg_prof_kernels()
        names = [L.dsvg_prof_kernel_name(i).decode() for i in range(nk)]
        watched = [i for i, n in enumerate(names) if "k_pack_n" in n or "k_pixout" in n]
        for name, pf, osub in settings:
            assert L.dsvg_prof_enable(d.ctx, sum(1 << i for i in watched)) == 0 and L.dsvg_prof_reset(d.ctx) == 0
            one_run(name, pf, osub)
            for i in watched:
                ms, n, by = C.c_double(0), C.c_long(0), C.c_double(0)
                assert L.dsvg_prof_get(d.ctx, i, C.byref(ms), C.byref(n), C.byref(by)) == 0
                if n.value:
                    print("  %-38s %s: %d launches, %.1f us each, %.2f MB read + written each, %.0f GB/s" %
                          (name, names[i], n.value, ms.value / n.value * 1e3, by.value / n.value / 1e6, by.value / ms.value / 1e6))
            assert L.dsvg_prof_enable(d.ctx, 0) == 0
        d.close()


if "--formats" in sys.argv[1:]:
    output_formats(int(os.environ.get("DEC_STREAMS", "64")))
    sys.exit(0)
clip = A.gen_clip(W, H, FMT, 0x10800003, 12, style=0)
clip = np.concatenate([clip] * (N // 12), axis=0)
stream = pkg.encode_clip(clip, W, H, FMT, qp=85, gop=12, rc_mode_cli=1)
pk = A.split_packets(stream)


class Decoder(C.Structure):
    _fields_ = [("vidmeta", A.Meta), ("ref", C.c_void_p), ("draw_info", C.c_int), ("got_metadata", C.c_int)]


L.dsv_alloc.restype = C.c_void_p
L.dsv_dec.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
L.dsv_frame_ref_dec.argtypes = [C.c_void_p]
L.dsv_frame_ref_dec.restype = None
for rep in range(3):
    dec = Decoder()
    # the packets as a C caller has them: in dsv_alloc'd buffers (dsv_dec frees them), prepared before the clock starts
    bufs = []
    LOOPS = 10                                         # the stream ten times over through ONE decoder (its end-of-stream packet left out): the
    for p in [q for q in pk if q[5] != 0x10] * LOOPS:  # session's set-up (context, pinned frames: ~15 ms) is not what the figure is about
        buf = pkg.Buf()
        mem = L.dsv_alloc(len(p)); C.memmove(mem, p, len(p))
        buf.data = C.cast(mem, C.POINTER(C.c_uint8)); buf.len = len(p)
        bufs.append(buf)
    frame = C.c_void_p(None); fn = C.c_uint32(0)
    dref, bref, fref, nref = C.byref(dec), [C.byref(b) for b in bufs], C.byref(frame), C.byref(fn)
    t0 = time.perf_counter(); n = 0
    for br in bref:
        frame.value = None
        rc = L.dsv_dec(dref, br, fref, nref)
        if rc == 0 and frame.value:
            n += 1; L.dsv_frame_ref_dec(frame)
    dt = time.perf_counter() - t0
    L.dsv_dec_free(C.byref(dec))
print("dsv_dec, one picture per call, host frame out: %d frames 1920x1080 decoded in %.3f s: %.0f frames/s, %.2f Gpix/s (stream %d bytes)" % (n, dt, n / dt, n * W * H / dt / 1e9, len(stream)))

# ---- batched decoder (dsv1_decbatch_*): S copies of the stream side by side, one packet per stream per call ----
S = int(os.environ.get("DEC_STREAMS", "64"))
for on_device in (1, 0):
    d = pkg.DecBatch(W, H, FMT, S)
    keep = [np.frombuffer(bytes(p) + b"\0" * 16, dtype=np.uint8).copy() for p in pk]
    calls = []
    for k, p in enumerate(pk):
        bufs = (pkg.Buf * S)()
        for s in range(S):
            bufs[s].data = keep[k].ctypes.data_as(C.POINTER(C.c_uint8)); bufs[s].len = len(p)
        calls.append(bufs)
    status = (C.c_int * S)(); fnum = (C.c_uint32 * S)()
    if on_device:
        dst = C.c_void_p(None)
        assert L.dsvg_dev_alloc(d.ctx, C.byref(dst), d.frame_bytes * S) == 0
    else:
        b = pkg.Batch(pkg.make_encoder_cfg(W, H, FMT), 1, 1)
        host = b.pinned((S, d.frame_bytes))
        dst = C.c_void_p(host.ctypes.data)
    for rep in range(2):
        d.sync()
        t0 = time.perf_counter(); n = 0
        for bufs in calls:
            rc = L.dsv1_decbatch_decode(d.h, bufs, dst, d.frame_bytes, on_device, status, fnum)
            assert rc == 0, L.dsvg_last_error()
            n += sum(1 for s in range(S) if status[s] == 0 and fnum[s] != 0xFFFFFFFF)
        d.sync()
        dt = time.perf_counter() - t0
    print("batched, %d streams, output %s: %d frames in %.3f s: %.0f frames/s, %.2f Gpix/s" %
          (S, "left in HBM" if on_device else "copied to pinned host memory", n, dt, n / dt, n * W * H / dt / 1e9))
    if on_device:
        L.dsvg_dev_free(d.ctx, dst)
    d.close()
