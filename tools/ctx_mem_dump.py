"""What a context's memory costs, without a device (dsvg_ctx_mem_plan, csrc/dsvg_ctx_mem.h).
    python tools/ctx_mem_dump.py W H SUBSAMP PYRAMID N_SRC N_RECON MAX_JOBS OUT_SLOTS [BLK_W BLK_H]     the table of one context
    python tools/ctx_mem_dump.py --design      the two tables of DESIGN.md: the headline encoder context, the 64-stream batched decoder's
    python tools/ctx_mem_dump.py --raw         the three contexts of tools/ctx_mem_host.cpp, in that program's format
SUBSAMP: 0 = 4:4:4, 4 = 4:2:2, 5 = 4:2:0, 8 = 4:1:1; PYRAMID 0: the encoder's own depth."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("digital-subband-video-1_amd")

HEADLINE = (1920, 1080, 5, 0, 25 * 320, 2 * 320, 320, 2 * 320 * 12)      # bench.py: 320 GOPs of 12 frames (dsv1_batch_open's slots)
DECODER64 = (1920, 1080, 5, 1, 1, 3 * 64, 64, 64)                        # dsv1_decbatch_open, 64 streams
# buffers no decoder call touches (dsvg_decode_pictures, the output pass, the downloads): the encoder's analysis, entropy pack and
# rate control, and what is staged for them
ENCODER_ONLY = ("src0", "src1", "chunks", "cflag", "llsym", "psum", "bits", "rc_state_d", "rcj_d", "rcj_h", "mvf", "aux_tex",
                "aux_var", "csum", "luma_sums", "gtab_d", "gtab_h", "psum_h", "luma_h", "aslots_h", "amv_h", "slot_cu_h", "slot_cv_h", "slot_cs_h",
                "slot_cu_d", "slot_cv_d", "slot_cs_d", "slot_y_h", "slot_y_d")
RAW = ((96, 64, 5, 0, 2, 3, 2, 4, 0, 0), (250, 130, 4, 2, 24, 24, 16, 48, 0, 0), (1920, 1080, 5, 1, 1, 192, 64, 64, 0, 0))
NEEDS = (1, 4095, 196672, (1 << 20) + 1, 64 << 20)


def table(args, out=sys.stdout):
    rows, tot = pkg.ctx_mem_plan(*args)
    out.write("| buffer | kind | elements | size | pad | zeroed | bytes |\n|---|---|---:|---:|---:|---|---:|\n")
    for r in rows:
        out.write("| %s | %s | %d | %d | %d | %s | %d |\n" % (r["name"], r["kind"], r["count"], r["size"], r["pad"], "yes" if r["zeroed"] else "no", r["bytes"]))
    out.write("\ndevice %d bytes (%.2f GiB), pinned %d bytes (%.2f MiB), %d buffers\n" % (tot["device"], tot["device"] / 2**30, tot["pinned"], tot["pinned"] / 2**20, len(rows)))
    return rows, tot


def raw(out=sys.stdout):
    names = pkg.ctx_mem_names()
    for a in RAW:
        rows, tot = pkg.ctx_mem_plan(*a)
        out.write("ctx %s: %d rows, device %d, pinned %d\n" % (" ".join(map(str, a)), len(rows), tot["device"], tot["pinned"]))
        for r in rows:
            out.write("%s %d %d %d %d %d %d\n" % (r["name"], pkg.MEM_KINDS.index(r["kind"]), r["count"], r["size"], r["pad"], int(r["zeroed"]), r["bytes"]))
        geo = dict(zip(("w", "h", "fmt", "pyramid_levels", "n_src_slots", "n_recon_slots", "max_jobs", "out_slots", "blk_w", "blk_h"), a))
        for name in names[names.index("ltab_d"):]:
            for need in NEEDS:
                for few in (0, 1):
                    out.write("%s need %d few %d: %d %d\n" % (name, need, few, pkg.ctx_mem_grow(name, need, 0, few=few, **geo), pkg.ctx_mem_grow(name, need, 4096, few=few, **geo)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--raw"]:
        raw()
    elif sys.argv[1:] == ["--design"]:
        print("Headline encoder context: 1080p 4:2:0, n_src %d, n_recon %d, max_jobs %d, out_slots %d\n" % HEADLINE[4:])
        table(HEADLINE)
        print("\nBatched decoder context, 64 streams: 1080p 4:2:0, pyramid 1, n_src %d, n_recon %d, max_jobs %d, out_slots %d\n" % DECODER64[4:])
        rows, tot = table(DECODER64)
        idle = [r for r in rows if r["name"] in ENCODER_ONLY]
        print("\nNo decoder call touches: %s -- %d bytes (%.2f GiB) of the device total, %d bytes pinned" % (
            ", ".join("%s (%d)" % (r["name"], r["bytes"]) for r in idle), sum(r["bytes"] for r in idle if r["kind"] != "pinned"),
            sum(r["bytes"] for r in idle if r["kind"] != "pinned") / 2**30, sum(r["bytes"] for r in idle if r["kind"] == "pinned")))
    elif len(sys.argv) in (9, 11):
        table(tuple(int(x, 0) for x in sys.argv[1:]))
    else:
        sys.exit(__doc__)
