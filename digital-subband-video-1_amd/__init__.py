"""MI355X-native DSV1 hot path: thin ctypes binding over the C ABI (include/dsvg.h, include/dsv1_api.h).

The product is libdsv1_mi355x.so (HIP kernels for gfx950 + the C session layer).  This module only
loads it and marshals arguments; there is no Python or CPU fallback -- if the library is missing,
or no HIP device is usable, calls fail loudly."""
import ctypes as _C
import os as _os

import numpy as _np

_HERE = _os.path.dirname(_os.path.abspath(__file__))
# DSV1_SO: another build of the same library (A/B variants of tools/ab/variants.sh); never a different implementation
SO_PATH = _os.environ.get("DSV1_SO") or _os.path.join(_HERE, "libdsv1_mi355x.so")
_lib = None

SUBSAMP_444, SUBSAMP_422, SUBSAMP_420, SUBSAMP_411 = 0x0, 0x4, 0x5, 0x8
MAX_QUALITY = 2047


class Meta(_C.Structure):
    _fields_ = [("width", _C.c_int), ("height", _C.c_int), ("subsamp", _C.c_int), ("fps_num", _C.c_int),
                ("fps_den", _C.c_int), ("aspect_num", _C.c_int), ("aspect_den", _C.c_int)]


class Encoder(_C.Structure):
    """DSV_ENCODER (dsv_encoder.h:58-110 field order)"""
    _fields_ = [("quality", _C.c_int), ("gop", _C.c_int), ("do_scd", _C.c_int), ("rc_mode", _C.c_int),
                ("rc_high_motion_nudge", _C.c_int), ("bitrate", _C.c_uint), ("max_q_step", _C.c_int),
                ("min_quality", _C.c_int), ("max_quality", _C.c_int), ("min_I_frame_quality", _C.c_int),
                ("intra_pct_thresh", _C.c_int), ("scene_change_delta", _C.c_int), ("stable_refresh", _C.c_uint),
                ("pyramid_levels", _C.c_int),
                ("rc_quant", _C.c_uint), ("bpf_total", _C.c_uint), ("bpf_reset", _C.c_uint), ("bpf_avg", _C.c_int),
                ("total_P_frame_q", _C.c_int), ("avg_P_frame_q", _C.c_int), ("last_P_frame_over", _C.c_int),
                ("back_into_range", _C.c_int), ("next_fnum", _C.c_uint32), ("ref", _C.c_void_p), ("vidmeta", Meta),
                ("prev_link", _C.c_int), ("force_metadata", _C.c_int), ("stability", _C.c_void_p),
                ("refresh_ctr", _C.c_uint), ("stable_blocks", _C.c_void_p), ("prev_gop", _C.c_uint32),
                ("prev_avg_luma", _C.c_int)]


class Buf(_C.Structure):
    _fields_ = [("data", _C.POINTER(_C.c_uint8)), ("len", _C.c_uint)]


class Dispatch(_C.Structure):
    """dsvg_dispatch (include/dsvg.h): the branches the encoder's forward launchers take"""
    _fields_ = [("blk_w", _C.c_int), ("blk_h", _C.c_int), ("fusable", _C.c_int), ("fwd", _C.c_int * 2), ("hme_levels", _C.c_int),
                ("hme", (_C.c_int * 4) * 6), ("csum", _C.c_int), ("tail_threads", _C.c_int), ("scan_threads", _C.c_int)]

    def as_dict(self):
        n = self.hme_levels + 1
        return {"blk": (self.blk_w, self.blk_h), "fusable": self.fusable, "fwd": tuple(self.fwd), "csum": self.csum, "threads": (self.tail_threads, self.scan_threads),
                "hme": tuple(tuple(self.hme[l]) for l in range(max(n, 0)))}


INV_NO_PATCH_PART, INV_NO_EDGE_TILES, INV_NO_FUSED_BORDER, INV_NO_XCD_ORDER = 1, 2, 4, 8      # DSVG_INV_NO_*
INV_COVER_NONE, INV_COVER_WHOLE, INV_COVER_RECT, INV_COVER_FROM = 0, 1, 2, 3                 # DSVG_INV_COVER_*


class InvStep(_C.Structure):
    """dsvg_inv_step (include/dsvg.h): one launch of the inverse transform's plan"""
    _fields_ = [("kernel", _C.c_int), ("grid", _C.c_int * 3), ("xcd", _C.c_int), ("args", _C.c_int * 4), ("bytes", _C.c_double),
                ("cover", _C.c_int), ("cx", _C.c_int), ("cy", _C.c_int)]

    def as_dict(self):
        return {"kernel": lib().dsvg_prof_kernel_name(self.kernel).decode(), "grid": tuple(self.grid), "xcd": self.xcd, "args": tuple(self.args),
                "bytes": self.bytes, "cover": (self.cover, self.cx, self.cy)}


FWD_GROUP_STEP = 2                                                                           # DSVG_FWD_GROUP_STEP
FWD_NO_XCD_ORDER, FWD_NO_MC_FUSION, FWD_NO_LLQ = 1, 2, 4                                     # DSVG_FWD_NO_*


class FwdStep(_C.Structure):
    """dsvg_fwd_step (include/dsvg.h): one launch of the forward transform's plan"""
    _fields_ = [("kernel", _C.c_int), ("grid", _C.c_int * 3), ("xcd", _C.c_int), ("block", _C.c_int * 2), ("lds", _C.c_uint),
                ("args", _C.c_int * 4), ("bytes", _C.c_double)]

    def as_dict(self):
        return {"kernel": lib().dsvg_prof_kernel_name(self.kernel).decode(), "grid": tuple(self.grid), "xcd": self.xcd,
                "block": tuple(self.block), "lds": self.lds, "args": tuple(self.args), "bytes": self.bytes}


class HmeStep(_C.Structure):
    """dsvg_hme_step (include/dsvg.h): one launch of the motion search's plan"""
    _fields_ = [("kernel", _C.c_int), ("l0", _C.c_int), ("nkbf", _C.c_int), ("part", _C.c_int), ("level", _C.c_int), ("count", _C.c_int),
                ("fullx", _C.c_int), ("fully", _C.c_int), ("inv_per", _C.c_uint), ("inv_row", _C.c_uint), ("grid", _C.c_int * 2),
                ("block", _C.c_int), ("bytes", _C.c_double), ("cont", _C.c_int)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("l0", "nkbf", "part", "level", "count", "fullx", "fully", "inv_per", "inv_row", "block", "bytes", "cont")}
        d.update(kernel=lib().dsvg_prof_kernel_name(self.kernel).decode(), grid=tuple(self.grid))
        return d


BATCH_NO_SMALL_SPLIT, BATCH_NO_PAR_ENQUEUE, BATCH_NO_LAZY_BORDER, BATCH_NO_MC_FUSION, BATCH_PROFILED = 1, 2, 4, 8, 16      # DSVG_BATCH_*
DEC_NO_SYM, DEC_NO_SYM_I, DEC_ONE_STREAM, DEC_NO_MC_PATCH, DEC_NO_INPLACE_PRED, DEC_NO_SYM_OV, DEC_NO_MC_FUSION, DEC_PROFILED = (
    1, 2, 4, 8, 16, 32, 64, 128)                                                                                           # DSVG_DEC_*


LOAD_NO_UNPACK_SIDES, LOAD_NO_LEVEL_SIDES, LOAD_NO_FUSE_LEVEL2 = 1, 2, 4                                                  # DSVG_LOAD_NO_*
UNPACK_BODIES = ("none", "scalar", "v16", "fused1", "fused2")                                                              # DSVG_UNPACK_*
BORDER_KERNELS = (None, "k_extend", "k_extend16")                                                                          # DSVG_BORDER_*
LOAD_KERNELS = ("k_unpack", "k_extend", "k_extend16", "k_ds2x", "k_luma_sum")                                              # kernel ids 0..4


class LoadLevel(_C.Structure):
    """dsvg_load_level (include/dsvg.h): one level of a source load's plan"""
    _fields_ = [(k, _C.c_int) for k in ("w", "h", "border", "tb_only", "ds2x", "ds2x_sides", "ds2x_tail", "src_odd_w", "src_odd_h")]


class LoadPlan(_C.Structure):
    """dsvg_load_plan_out (include/dsvg.h): the plan of a source load"""
    _fields_ = [("levels", _C.c_int), ("sides", _C.c_int), ("fuse1", _C.c_int), ("fuse2", _C.c_int), ("sides1", _C.c_int), ("sides2", _C.c_int),
                ("body", _C.c_int * 3), ("grid_planes", _C.c_int), ("level", LoadLevel * 6), ("luma_sum", _C.c_int), ("luma_sum_dword", _C.c_int),
                ("ring_x16", _C.c_int), ("ring_y4", _C.c_int), ("chroma_in_place_ok", _C.c_int), ("luma_in_place_ok", _C.c_int),
                ("launches", _C.c_int * 5), ("bytes", _C.c_double * 5)]


class PicJob(_C.Structure):
    """dsvg_pic_job (include/dsvg.h): one picture of a coding call"""
    _fields_ = [("src_slot", _C.c_int), ("ref_recon_slot", _C.c_int), ("recon_slot", _C.c_int), ("quant", _C.c_int), ("mvs", _C.c_void_p),
                ("stable_blocks", _C.c_void_p), ("out_slot", _C.c_int), ("no_intra_blocks", _C.c_int), ("has_reach", _C.c_int),
                ("mv_reach", _C.c_short * 4), ("border_hint", _C.c_int)]


class RcJob(_C.Structure):
    """dsvg_rc_job (include/dsvg.h): the rate-controlled stream a picture of a coding call belongs to"""
    _fields_ = [("rc_slot", _C.c_int), ("prefix_len", _C.c_int), ("forced_intra", _C.c_int)]


class BatchPlan(_C.Structure):
    """dsvg_batch_plan (include/dsvg.h): the plan of a coding call, arrays of the caller's"""
    _fields_ = [("cap_steps", _C.c_int), ("cap_jobs", _C.c_int), ("cap_groups", _C.c_int), ("cap_ilist", _C.c_int),
                ("nI", _C.c_void_p), ("order", _C.c_void_p), ("mvu", _C.c_void_p), ("stu", _C.c_void_p), ("mvcp", _C.c_void_p),
                ("stcp", _C.c_void_p), ("ext", _C.c_void_p), ("rc_next", _C.c_void_p), ("ioff", _C.c_void_p), ("icnt", _C.c_void_p),
                ("noint", _C.c_void_p), ("keeps", _C.c_void_p), ("ilist", _C.c_void_p),
                ("nblk", _C.c_int), ("mc_fused", _C.c_int), ("base", _C.c_int), ("total", _C.c_int), ("ng", _C.c_int), ("gk", _C.c_int * 5),
                ("iln", _C.c_int), ("nmv", _C.c_int), ("nst", _C.c_int), ("mv_contig", _C.c_int), ("par_enqueue", _C.c_int)]


class BatchRefused(RuntimeError):
    """dsvg_code_batch_plan did not answer with a plan: rc and text are what the coding call itself would return and set"""
    def __init__(self, rc, text):
        super().__init__("dsvg_code_batch_plan failed rc=%d: %s" % (rc, text))
        self.rc, self.text = rc, text


class DecJob(_C.Structure):
    """dsvg_dec_job (include/dsvg.h): one picture of a decoder call"""
    _fields_ = [("ref_recon_slot", _C.c_int), ("recon_slot", _C.c_int), ("quant", _C.c_int), ("mvs", _C.c_void_p), ("stable_blocks", _C.c_void_p),
                ("plane_data", _C.c_void_p * 3), ("plane_len", _C.c_uint32 * 3)]


MV_DTYPE = _np.dtype({"names": ["x", "y", "mode", "submask", "lo_var", "lo_tex", "high_detail"], "formats": ["<i2", "<i2", "u1", "u1", "u1", "u1", "u1"],
                      "offsets": [0, 2, 4, 5, 6, 7, 8], "itemsize": 12})      # dsvg_mv (its union holds an int32: 12 bytes)


class DecPlan(_C.Structure):
    """dsvg_dec_plan (include/dsvg.h): the plan of a decoder call, arrays of the caller's"""
    _fields_ = [("cap_jobs", _C.c_int), ("cap_ilist", _C.c_int), ("order", _C.c_void_p), ("path", _C.c_void_p), ("dec_sym", _C.c_void_p),
                ("wide", _C.c_void_p), ("inplace", _C.c_void_p), ("dc", _C.c_void_p), ("runs", _C.c_void_p), ("len", _C.c_void_p),
                ("bitpos", _C.c_void_p), ("blob_off", _C.c_void_p), ("meta_off", _C.c_void_p), ("ilist", _C.c_void_p),
                ("nblk", _C.c_int), ("nbh", _C.c_int), ("mc_patch", _C.c_int), ("sym_ok", _C.c_int * 2), ("ov", _C.c_int * 2),
                ("second_stream", _C.c_int), ("nchunks", _C.c_int * 3), ("lim", (_C.c_int * 16) * 2), ("nI", _C.c_int),
                ("blob", _C.c_longlong), ("nmeta", _C.c_longlong), ("max_entries", _C.c_int), ("max_chunks", _C.c_int),
                ("insym", _C.c_int), ("f0", _C.c_int), ("anysym", _C.c_int), ("scatter_one", _C.c_int), ("resolve", _C.c_int), ("fork", _C.c_int),
                ("mc", _C.c_int), ("ex0", _C.c_int), ("ey0", _C.c_int), ("iln", _C.c_int), ("draw0", _C.c_int), ("draw1", _C.c_int)]


class DecodeRefused(RuntimeError):
    """dsvg_decode_plan did not answer with a plan: rc and text are what the decoder call itself would return and set"""
    def __init__(self, rc, text):
        super().__init__("dsvg_decode_plan failed rc=%d: %s" % (rc, text))
        self.rc, self.text = rc, text


class ResRung(_C.Structure):
    """dsv1_res_rung: one geometry of a resolution ladder and its rate rungs"""
    _fields_ = [("width", _C.c_int), ("height", _C.c_int), ("nrates", _C.c_int), ("rates", _C.POINTER(Encoder))]


PIX_PLANAR, PIX_SEMIPLANAR_UV, PIX_SEMIPLANAR_VU, PIX_PACKED_YUYV, PIX_PACKED_UYVY = 0, 1, 2, 3, 4   # DSV1_PIX_*


class PixFormat(_C.Structure):
    """dsv1_pix_format: how a source clip lies in memory -- layout (PIX_*), depth (8, 10, 12, 16; above 8: little-endian 16-bit words),
    msb_aligned (P010: 1, yuv420p10le: 0), row pitches in bytes (0 = tight) and the bytes from frame to frame (0 = tight)"""
    _fields_ = [("layout", _C.c_int), ("depth", _C.c_int), ("msb_aligned", _C.c_int), ("pitch", _C.c_int * 3), ("frame_bytes", _C.c_size_t)]

    def __init__(self, layout=PIX_PLANAR, depth=8, msb_aligned=0, pitch=(0, 0, 0), frame_bytes=0):
        super().__init__(layout, depth, msb_aligned, (_C.c_int * 3)(*pitch), frame_bytes)


RGB_RGB24, RGB_BGR24, RGB_RGBA, RGB_BGRA, RGB_ARGB, RGB_ABGR, RGB_PLANAR_RGB, RGB_PLANAR_GBR = range(8)   # DSV1_RGB_*
MATRIX_BT601, MATRIX_BT709, MATRIX_BT2020 = 0, 1, 2   # DSV1_MATRIX_*
CHROMA_REPLICATE, CHROMA_LINEAR = 0, 1   # DSV1_CHROMA_*


class RgbFormat(_C.Structure):
    """dsv1_rgb_format: 8-bit RGB frames -- order (RGB_*), matrix (MATRIX_*), full_range (0: 16..235 / 16..240, 1: 0..255), upsample
    (CHROMA_*: how chroma reaches the luma grid on output), row pitches in bytes (0 = tight) and the bytes from frame to frame (0 =
    tight)"""
    _fields_ = [("order", _C.c_int), ("matrix", _C.c_int), ("full_range", _C.c_int), ("upsample", _C.c_int), ("pitch", _C.c_int * 3),
                ("frame_bytes", _C.c_size_t)]

    def __init__(self, order=RGB_RGB24, matrix=MATRIX_BT709, full_range=0, upsample=CHROMA_LINEAR, pitch=(0, 0, 0), frame_bytes=0):
        super().__init__(order, matrix, full_range, upsample, (_C.c_int * 3)(*pitch), frame_bytes)


TRANSFER_PQ, TRANSFER_HLG = 0, 1   # DSV1_TRANSFER_*
TONEMAP_CLIP, TONEMAP_REINHARD, TONEMAP_BT2390 = 0, 1, 2   # DSV1_TONEMAP_*
HDR_ONE, HDR_NBUCKETS = 1 << 20, 3329


class Hdr(_C.Structure):
    """dsv1_hdr: the settings of an HDR import -- transfer (TRANSFER_*), matrix / full_range of the source signal, gamut (1: BT.2020
    primaries to BT.709), curve (TONEMAP_*), peak_nits 100..10000, white_nits (the HDR level that becomes SDR 1.0; 0 = 203),
    out_matrix / out_full_range of the SDR signal.  hdr_build makes the tables of them; include/dsv1_api.h, HDR sources, has the
    definition."""
    _fields_ = [(k, _C.c_int) for k in ("transfer", "matrix", "full_range", "gamut", "curve", "peak_nits", "white_nits", "out_matrix",
                                        "out_full_range")]

    def __init__(self, transfer=TRANSFER_PQ, matrix=MATRIX_BT2020, full_range=0, gamut=1, curve=TONEMAP_BT2390, peak_nits=1000, white_nits=203,
                 out_matrix=MATRIX_BT709, out_full_range=0):
        super().__init__(transfer, matrix, full_range, gamut, curve, peak_nits, white_nits, out_matrix, out_full_range)


class HdrTables(_C.Structure):
    """dsv1_hdr_tables: what the HDR import's pixel path reads -- a plain struct a caller may edit (own curve, own look)"""
    _fields_ = [("ycc", _C.c_int32 * 5), ("in_oy", _C.c_int32), ("in_oc", _C.c_int32), ("eotf", _C.c_uint32 * 4096), ("gamut", _C.c_int32 * 9),
                ("gain", _C.c_uint32 * HDR_NBUCKETS), ("oetf", _C.c_uint16 * HDR_NBUCKETS), ("fwd", _C.c_int32 * 9), ("ybias", _C.c_int32),
                ("cbias", _C.c_int32)]

    def as_dict(self):
        """the tables as numpy arrays / ints (copies)"""
        return {k: (_np.array(getattr(self, k)[:]) if hasattr(getattr(self, k), "__len__") else int(getattr(self, k))) for k, _ in self._fields_}

    @classmethod
    def from_dict(cls, d):
        t = cls()
        for k, ty in cls._fields_:
            if hasattr(ty, "_length_"):
                getattr(t, k)[:] = [int(x) for x in d[k]]
            else:
                setattr(t, k, int(d[k]))
        return t


DEINT_FRAME, DEINT_FIELD = 0, 1


class Deint(_C.Structure):
    """dsv1_deint: the deinterlacer's mode (DEINT_FRAME: n frames in, n out; DEINT_FIELD: n in, 2n out) and the field order of the
    source (tff = 1: the top field is the earlier one).  include/dsv1_api.h, Deinterlacing, has the definition."""
    _fields_ = [("mode", _C.c_int), ("tff", _C.c_int)]

    def __init__(self, mode=DEINT_FRAME, tff=1):
        super().__init__(mode, tff)


IVTC_C, IVTC_P = 0, 1                    # DSV1_IVTC_*: a frame's match


class Ivtc(_C.Structure):
    """dsv1_ivtc: inverse telecine of 3:2 pulled-down film -- the field order of the source (tff = 1: the top field is the earlier
    one) and the comb measure's noise threshold nt (0 .. 254).  5n frames in, the 4n film frames out.  include/dsv1_api.h, Inverse
    telecine, has the definition."""
    _fields_ = [("tff", _C.c_int), ("nt", _C.c_int), ("reserved", _C.c_int * 2)]

    def __init__(self, tff=1, nt=0):
        super().__init__(tff, nt, (_C.c_int * 2)(0, 0))


class Denoise(_C.Structure):
    """dsv1_denoise: the temporal noise filter's strengths, luma for plane 0 and chroma for planes 1 and 2, each 0 .. 512 and not both
    0; a plane with strength 0 is copied.  include/dsv1_api.h, Temporal noise reduction, has the definition."""
    _fields_ = [("luma", _C.c_int), ("chroma", _C.c_int)]

    def __init__(self, luma=24, chroma=24):
        super().__init__(luma, chroma)


class Reframe(_C.Structure):
    """dsv1_reframe: the window (x, y, w, h) of in_w x in_h frames placed at (dst_x, dst_y) on a canvas of out_w x out_h, `fill`
    (Y, U, V) elsewhere: crop, pad, letterbox and pillarbox in one.  include/dsv1_api.h, Reframe, has the definition."""
    _fields_ = [("in_w", _C.c_int), ("in_h", _C.c_int), ("x", _C.c_int), ("y", _C.c_int), ("w", _C.c_int), ("h", _C.c_int),
                ("out_w", _C.c_int), ("out_h", _C.c_int), ("dst_x", _C.c_int), ("dst_y", _C.c_int), ("fill", _C.c_uint8 * 3),
                ("reserved", _C.c_uint8)]

    def __init__(self, in_w, in_h, window=None, out=None, dst=(0, 0), fill=(16, 128, 128)):
        """window: (x, y, w, h), None: the whole input; out: (out_w, out_h), None: the window's size"""
        x, y, w, h = window if window is not None else (0, 0, in_w, in_h)
        ow, oh = out if out is not None else (w, h)
        super().__init__(in_w, in_h, x, y, w, h, ow, oh, dst[0], dst[1], (_C.c_uint8 * 3)(*fill), 0)


class Orient:
    """the eight orientations (DSV1_ORIENT_*; include/dsv1_api.h, Orientation): bit 2 transposes first, bit 0 then mirrors the columns
    of the result, bit 1 its rows.  ROT90 and ROT270 are clockwise."""
    NONE, HFLIP, VFLIP, ROT180, TRANSPOSE, ROT90, ROT270, TRANSVERSE = range(8)


class Levels(_C.Structure):
    """dsv1_levels: three 256-entry tables, one per plane (Y, U, V), out_p[i] = lut[p][in_p[i]] (include/dsv1_api.h, Levels).  The
    builders are the library's host-only ones, exact integers: identity(), range(src_full, dst_full), adjust(...), a.compose(b) (a
    first).  Any other curve: fill .lut / from_tables()."""
    _fields_ = [("lut", (_C.c_uint8 * 256) * 3)]

    @classmethod
    def identity(cls):
        lv = cls()
        _chk(lib().dsv1_levels_identity(_C.byref(lv)), "dsv1_levels_identity")
        return lv

    @classmethod
    def range(cls, src_full, dst_full):
        """full-range (1) or limited-range (0) YCbCr in, the other (or the same: the identity) out (dsv1_levels_range)"""
        lv = cls()
        if lib().dsv1_levels_range(_C.byref(lv), int(src_full), int(dst_full)):
            raise ValueError("Levels.range(%r, %r): the flags are 0 or 1" % (src_full, dst_full))
        return lv

    @classmethod
    def adjust(cls, in_black=0, in_white=255, out_black=0, out_white=255, sat_q8=256):
        """black and white point of the luma, saturation of the chroma in 1/256 (dsv1_levels_adjust)"""
        lv = cls()
        if lib().dsv1_levels_adjust(_C.byref(lv), in_black, in_white, out_black, out_white, sat_q8):
            raise ValueError("Levels.adjust(%d, %d, %d, %d, %d) refused" % (in_black, in_white, out_black, out_white, sat_q8))
        return lv

    @classmethod
    def from_tables(cls, tables):
        """tables: anything numpy reads as uint8 [3][256]"""
        t = _np.ascontiguousarray(tables, dtype=_np.uint8)
        if t.shape != (3, 256):
            raise ValueError("levels are three tables of 256 entries")
        lv = cls()
        _C.memmove(_C.byref(lv), t.ctypes.data, 768)
        return lv

    def compose(self, then):
        """the tables equal to applying self and then `then` (dsv1_levels_compose)"""
        out = Levels()
        _chk(lib().dsv1_levels_compose(_C.byref(self), _C.byref(then), _C.byref(out)), "dsv1_levels_compose")
        return out

    def is_identity(self):
        return bool(lib().dsv1_levels_is_identity(_C.byref(self)))

    def tables(self):
        """numpy uint8 [3][256], a copy"""
        return _np.frombuffer(bytes(self), dtype=_np.uint8).reshape(3, 256).copy()


class Overlay(_C.Structure):
    """dsv1_overlay: one timed bitmap of an overlay list (include/dsv1_api.h, Overlays).  planes: numpy uint8, the bitmap's Y (w x h), U,
    V (chroma size of w x h at the session's subsampling) and A (w x h, straight alpha) one after the other -- overlay_from_rgba makes
    them from an RGBA image -- kept alive with the object; None leaves the pointer NULL.  x, y: top left on the canvas; source: -1 for
    every source; t0, dur: first picture and number of pictures (0: for ever); fade_in, fade_out in pictures (0 .. 65535); opacity
    0 .. 256."""
    _fields_ = [("planes", _C.c_void_p), ("w", _C.c_int), ("h", _C.c_int), ("x", _C.c_int), ("y", _C.c_int), ("source", _C.c_int),
                ("opacity", _C.c_int), ("t0", _C.c_int64), ("dur", _C.c_uint32), ("fade_in", _C.c_uint16), ("fade_out", _C.c_uint16),
                ("reserved", _C.c_int)]

    def __init__(self, planes, w, h, x=0, y=0, source=-1, t0=0, dur=0, fade_in=0, fade_out=0, opacity=256, reserved=0):
        if not 0 <= fade_in <= 65535 or not 0 <= fade_out <= 65535 or not 0 <= dur < 1 << 32:
            raise ValueError("Overlay: fade_in and fade_out are 0 .. 65535, dur 0 .. 2^32 - 1")
        self._keep = None if planes is None else _np.ascontiguousarray(planes, dtype=_np.uint8).reshape(-1)
        super().__init__(None if planes is None else self._keep.ctypes.data, w, h, x, y, source, opacity, t0, dur, fade_in, fade_out,
                         reserved)


class OverlayItem(_C.Structure):
    """dsv1_overlay_item: one item of a call's overlay plan (overlay_plan)"""
    _fields_ = [("overlay", _C.c_int), ("source", _C.c_int), ("frame", _C.c_int), ("op", _C.c_int), ("layer", _C.c_int)]


def _overlay_array(overlays):
    """(ctypes array of dsv1_overlay or None, n); the Overlay objects -- and so their bitmaps -- outlive the call that uses it"""
    ovs = list(overlays) if overlays is not None else []
    if not ovs:
        return None, 0
    arr = (Overlay * len(ovs))()
    for i, o in enumerate(ovs):
        _C.memmove(_C.byref(arr, i * _C.sizeof(Overlay)), _C.byref(o), _C.sizeof(Overlay))
    arr._keep = ovs
    return arr, len(ovs)


class BlockInfo(_C.Structure):
    """dsv1_blockinfo: one block's side information (packet_blockinfo, draw_info_clip)"""
    _fields_ = [("mvx", _C.c_int16), ("mvy", _C.c_int16), ("mode", _C.c_uint8), ("submask", _C.c_uint8), ("stable", _C.c_uint8),
                ("reserved", _C.c_uint8)]


BLOCKINFO_DTYPE = _np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("mode", "u1"), ("submask", "u1"), ("stable", "u1"), ("reserved", "u1")])


def lib():
    global _lib
    if _lib is None:
        if not _os.path.exists(SO_PATH):
            raise RuntimeError("HIP extension %s is not built; run __graft_entry__.build()" % SO_PATH)
        L = _C.CDLL(SO_PATH)
        L.dsvg_last_error.restype = _C.c_char_p
        L.dsv1_batch_open.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Encoder), _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_batch_close.argtypes = [_C.c_void_p]
        L.dsv1_ladder_open.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Encoder), _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_batch_rungs.argtypes = [_C.c_void_p]
        L.dsv1_batch_set_fnum.argtypes = [_C.c_void_p, _C.c_int, _C.c_uint32]
        L.dsv1_batch_dropped_recons.restype = _C.c_long
        L.dsv1_batch_recon_all.argtypes = [_C.c_void_p, _C.c_int]
        for f in ("batch_sse", "batch_ssim", "resladder_sse", "resladder_ssim"):
            getattr(L, "dsv1_%s_enable" % f).argtypes = [_C.c_void_p, _C.c_int]
        for f in ("batch_get_sse", "resladder_get_sse", "resladder_get_src_sse"):        # the quality figures (_figures): SSE uint64,
            getattr(L, "dsv1_" + f).argtypes = [_C.c_void_p, _C.POINTER(_C.c_uint64), _C.c_size_t]
        for f in ("batch_get_ssim", "resladder_get_ssim", "resladder_get_src_ssim"):     # SSIM_FX int64
            getattr(L, "dsv1_" + f).argtypes = [_C.c_void_p, _C.POINTER(_C.c_int64), _C.c_size_t]
        L.dsv1_batch_dropped_recons.argtypes = [_C.c_void_p, _C.POINTER(_C.c_long)]
        L.dsv1_batch_encode.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_int, _C.POINTER(Buf)]
        L.dsv1_batch_submit.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_int, _C.POINTER(Buf)]
        L.dsv1_batch_collect.argtypes = [_C.c_void_p, _C.POINTER(Buf)]
        L.dsv1_batch_eos.argtypes = [_C.c_void_p, _C.c_int, _C.POINTER(Buf)]
        L.dsv1_concat_gops.argtypes = [_C.POINTER(Buf), _C.c_int, _C.POINTER(Buf)]
        L.dsv1_batch_ctx.restype = _C.c_void_p
        L.dsv1_batch_ctx.argtypes = [_C.c_void_p]
        L.dsv_free.argtypes = [_C.c_void_p]
        L.estimate_bitrate.restype = _C.c_uint
        L.estimate_bitrate.argtypes = [_C.c_int, _C.c_int, _C.POINTER(Meta)]
        L.dsvg_dev_alloc.argtypes = [_C.c_void_p, _C.POINTER(_C.c_void_p), _C.c_size_t]
        L.dsvg_dev_free.argtypes = [_C.c_void_p, _C.c_void_p]
        L.dsvg_dev_upload.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_void_p, _C.c_size_t]
        L.dsvg_ctx_sync.argtypes = [_C.c_void_p]
        L.dsvg_ctx_code_streams.argtypes = [_C.c_void_p, _C.c_int]
        L.dsvg_ctx_streams_apart.argtypes = [_C.c_void_p]
        L.dsvg_ctx_copy_queue.argtypes = [_C.c_void_p]
        L.dsvg_ctx_stream.restype = _C.c_void_p
        L.dsvg_ctx_stream.argtypes = [_C.c_void_p]
        L.dsvg_ctx_join.argtypes = [_C.c_void_p, _C.c_void_p]
        L.dsvg_ctx_tile_stats.argtypes = [_C.c_void_p, _C.POINTER(_C.c_ulonglong), _C.c_int]
        L.dsvg_ctx_tile_stats2.argtypes = [_C.c_void_p, _C.POINTER(_C.c_ulonglong), _C.c_int]
        L.dsvg_dev_download.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_void_p, _C.c_size_t]
        L.dsvg_host_alloc.argtypes = [_C.c_void_p, _C.POINTER(_C.c_void_p), _C.c_size_t]
        L.dsvg_host_free.argtypes = [_C.c_void_p, _C.c_void_p]
        L.dsv1_batch_stage.argtypes = [_C.c_void_p, _C.c_void_p]
        L.dsv1_decbatch_open.argtypes = [_C.POINTER(_C.c_void_p), _C.c_int, _C.POINTER(Meta), _C.c_int]
        L.dsv1_decbatch_decode.argtypes = [_C.c_void_p, _C.POINTER(Buf), _C.c_void_p, _C.c_size_t, _C.c_int,
                                           _C.POINTER(_C.c_int), _C.POINTER(_C.c_uint32)]
        L.dsv1_decbatch_close.argtypes = [_C.c_void_p]
        L.dsv1_decbatch_ctx.restype = _C.c_void_p
        L.dsv1_decbatch_ctx.argtypes = [_C.c_void_p]
        L.dsvg_prof_enable.argtypes = [_C.c_void_p, _C.c_ulonglong]
        L.dsvg_ctx_mark.argtypes = [_C.c_void_p, _C.c_int]
        L.dsvg_ctx_mark_ms.argtypes = [_C.c_void_p, _C.POINTER(_C.c_float)]
        L.dsvg_ctx_timeline.argtypes = [_C.c_void_p, _C.c_int]
        L.dsvg_ctx_timeline_get.argtypes = [_C.c_void_p, _C.POINTER(_C.c_double)]
        L.dsvg_ctx_fetch_prof.argtypes = [_C.c_void_p, _C.POINTER(_C.c_double), _C.c_int]
        L.dsv1_host_prof_enable.argtypes = [_C.c_int]
        L.dsv1_host_prof_enable.restype = None
        L.dsv1_host_prof_get.argtypes = [_C.POINTER(_C.c_double), _C.c_int, _C.POINTER(_C.c_long)]
        L.dsv1_host_prof_name.restype = _C.c_char_p
        L.dsv1_host_prof_name.argtypes = [_C.c_int]
        L.dsvg_link_probe.argtypes = [_C.c_int, _C.c_size_t, _C.c_int, _C.POINTER(_C.c_double)]
        L.dsv1_batch_encoder.restype = _C.c_void_p
        L.dsv1_batch_encoder.argtypes = [_C.c_void_p, _C.c_int]
        L.dsvg_prof_reset.argtypes = [_C.c_void_p]
        L.dsvg_prof_get.argtypes = [_C.c_void_p, _C.c_int, _C.POINTER(_C.c_double), _C.POINTER(_C.c_long),
                                    _C.POINTER(_C.c_double)]
        L.dsvg_prof_kernel_name.restype = _C.c_char_p
        L.dsv1_scale_taps.argtypes = [_C.c_int, _C.c_int, _C.c_int]
        L.dsv1_scale_weights.argtypes = [_C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_void_p, _C.c_int]
        L.dsv1_scale_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int, _C.c_int,
                                      _C.c_int, _C.c_int]
        L.dsv1_resladder_open.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.POINTER(ResRung), _C.c_int, _C.c_int, _C.c_int,
                                          _C.c_int, _C.c_int]
        L.dsv1_resladder_close.argtypes = [_C.c_void_p]
        L.dsv1_resladder_close.restype = None
        L.dsv1_resladder_nstreams.argtypes = [_C.c_void_p]
        L.dsv1_resladder_batch.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_resladder_batch.restype = _C.c_void_p
        L.dsv1_resladder_encoder.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_resladder_encoder.restype = _C.c_void_p
        for f in ("encode", "submit"):
            getattr(L, "dsv1_resladder_" + f).argtypes = [_C.c_void_p, _C.c_void_p, _C.c_int, _C.POINTER(Buf)]
        L.dsv1_resladder_collect.argtypes = [_C.c_void_p, _C.POINTER(Buf)]
        L.dsv1_resladder_eos.argtypes = [_C.c_void_p, _C.c_int, _C.POINTER(Buf)]
        L.dsv1_resladder_uploads.argtypes = [_C.c_void_p, _C.POINTER(_C.c_uint64), _C.POINTER(_C.c_long)]
        L.dsv1_resample_taps.argtypes = [_C.c_int, _C.c_int, _C.c_int]
        L.dsv1_resample_weights.argtypes = [_C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_void_p, _C.c_int]
        L.dsv1_resample_clip.argtypes = L.dsv1_scale_clip.argtypes
        L.dsv1_resladder_src_quality_enable.argtypes = [_C.c_void_p, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_pix_frame_bytes.restype = _C.c_size_t
        L.dsv1_pix_frame_bytes.argtypes = [_C.POINTER(PixFormat), _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_convert_clip.argtypes = [_C.c_int, _C.c_void_p, _C.POINTER(PixFormat), _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int]
        L.dsv1_batch_set_source_format.argtypes = [_C.c_void_p, _C.POINTER(PixFormat)]
        L.dsv1_resladder_open_src.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.POINTER(PixFormat), _C.POINTER(ResRung), _C.c_int,
                                              _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_decbatch_set_output_format.argtypes = [_C.c_void_p, _C.POINTER(PixFormat), _C.c_int]
        L.dsv1_decbatch_out_frame_bytes.restype = _C.c_size_t
        L.dsv1_decbatch_out_frame_bytes.argtypes = [_C.c_void_p]
        L.dsv1_export_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.POINTER(PixFormat), _C.c_int, _C.c_int]
        L.dsv1_convert_clip_sub.argtypes = [_C.c_int, _C.c_void_p, _C.POINTER(PixFormat), _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p,
                                            _C.c_int]
        L.dsv1_batch_set_source_format_sub.argtypes = [_C.c_void_p, _C.POINTER(PixFormat), _C.c_int]
        L.dsv1_resladder_open_src_sub.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.POINTER(PixFormat), _C.c_int, _C.POINTER(ResRung),
                                                  _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_export_clip_up.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.POINTER(PixFormat), _C.c_int,
                                          _C.c_int, _C.c_int]
        L.dsv1_decbatch_set_output_format_up.argtypes = [_C.c_void_p, _C.POINTER(PixFormat), _C.c_int, _C.c_int]
        L.dsv1_rgb_frame_bytes.restype = _C.c_size_t
        L.dsv1_rgb_frame_bytes.argtypes = [_C.POINTER(RgbFormat), _C.c_int, _C.c_int]
        L.dsv1_rgb_tables.argtypes = [_C.c_int, _C.c_int, _C.POINTER(_C.c_int32), _C.POINTER(_C.c_int32)]
        L.dsv1_rgb_import_clip.argtypes = [_C.c_int, _C.c_void_p, _C.POINTER(RgbFormat), _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int]
        L.dsv1_rgb_export_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.POINTER(RgbFormat), _C.c_int]
        L.dsv1_batch_set_source_rgb.argtypes = [_C.c_void_p, _C.POINTER(RgbFormat)]
        L.dsv1_resladder_open_rgb.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.POINTER(RgbFormat), _C.POINTER(ResRung), _C.c_int,
                                              _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_decbatch_set_output_rgb.argtypes = [_C.c_void_p, _C.POINTER(RgbFormat)]
        L.dsv1_hdr_valid.argtypes = [_C.POINTER(Hdr)]
        L.dsv1_hdr_build.argtypes = [_C.POINTER(Hdr), _C.POINTER(HdrTables)]
        L.dsv1_hdr_tables_valid.argtypes = [_C.POINTER(HdrTables)]
        L.dsv1_hdr_cidx_of.argtypes = [_C.c_uint32]
        L.dsv1_hdr_import_clip.argtypes = [_C.c_int, _C.c_void_p, _C.POINTER(PixFormat), _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p,
                                           _C.POINTER(HdrTables), _C.c_int, _C.c_int]
        L.dsv1_batch_set_source_hdr.argtypes = [_C.c_void_p, _C.POINTER(PixFormat), _C.c_int, _C.POINTER(HdrTables), _C.c_int]
        L.dsv1_resladder_open_hdr.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.POINTER(PixFormat), _C.c_int, _C.POINTER(HdrTables),
                                              _C.c_int, _C.POINTER(ResRung), _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_deint_out_frames.argtypes = [_C.POINTER(Deint), _C.c_int]
        L.dsv1_deinterlace_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_void_p,
                                            _C.POINTER(Deint), _C.c_int]
        L.dsv1_batch_set_source_deinterlace.argtypes = [_C.c_void_p, _C.POINTER(Deint)]
        L.dsv1_batch_deinterlace_reset.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_resladder_set_deinterlace.argtypes = [_C.c_void_p, _C.POINTER(Deint)]
        L.dsv1_resladder_deinterlace_reset.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_ivtc_out_frames.argtypes = [_C.POINTER(Ivtc), _C.c_int]
        L.dsv1_ivtc_state_bytes.argtypes = [_C.c_int, _C.c_int, _C.c_int]
        L.dsv1_ivtc_state_bytes.restype = _C.c_size_t
        L.dsv1_field_metrics_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int, _C.c_void_p,
                                              _C.c_int]
        L.dsv1_field_order_from_metrics.argtypes = [_C.c_void_p, _C.c_int, _C.c_int]
        L.dsv1_detect_field_order_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_ivtc_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_void_p, _C.c_void_p,
                                     _C.POINTER(Ivtc), _C.c_void_p, _C.c_void_p, _C.c_int]
        L.dsv1_batch_set_source_ivtc.argtypes = [_C.c_void_p, _C.POINTER(Ivtc)]
        L.dsv1_batch_ivtc_reset.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_resladder_set_ivtc.argtypes = [_C.c_void_p, _C.POINTER(Ivtc)]
        L.dsv1_resladder_ivtc_reset.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_denoise_state_bytes.argtypes = [_C.c_int, _C.c_int, _C.c_int]
        L.dsv1_denoise_state_bytes.restype = _C.c_size_t
        L.dsv1_denoise_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_void_p, _C.c_void_p,
                                        _C.POINTER(Denoise), _C.c_int]
        L.dsv1_batch_set_source_denoise.argtypes = [_C.c_void_p, _C.POINTER(Denoise)]
        L.dsv1_batch_denoise_reset.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_resladder_set_denoise.argtypes = [_C.c_void_p, _C.POINTER(Denoise)]
        L.dsv1_resladder_denoise_reset.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_reframe_valid.argtypes = [_C.POINTER(Reframe), _C.c_int]
        L.dsv1_reframe_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_void_p, _C.POINTER(Reframe), _C.c_int, _C.c_int]
        L.dsv1_line_sums_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_void_p, _C.c_int]
        L.dsv1_bars_from_sums.argtypes = [_C.c_void_p, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.POINTER(_C.c_int)]
        L.dsv1_detect_bars_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int,
                                            _C.POINTER(_C.c_int), _C.c_int]
        L.dsv1_batch_set_source_reframe.argtypes = [_C.c_void_p, _C.POINTER(Reframe)]
        L.dsv1_resladder_open_reframed.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.POINTER(Reframe), _C.POINTER(PixFormat),
                                                   _C.c_int, _C.POINTER(RgbFormat), _C.POINTER(ResRung), _C.c_int, _C.c_int, _C.c_int,
                                                   _C.c_int, _C.c_int]
        L.dsv1_orient_valid.argtypes = [_C.c_int, _C.c_int]
        L.dsv1_orient_dims.argtypes = [_C.c_int, _C.c_int, _C.c_int, _C.POINTER(_C.c_int), _C.POINTER(_C.c_int)]
        L.dsv1_orient_compose.argtypes = [_C.c_int, _C.c_int]
        L.dsv1_orient_inverse.argtypes = [_C.c_int]
        L.dsv1_orient_from_exif.argtypes = [_C.c_int]
        L.dsv1_orient_from_matrix.argtypes = [_C.POINTER(_C.c_int32)]
        L.dsv1_orient_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int, _C.c_int]
        L.dsv1_batch_set_source_orient.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_resladder_open_oriented.argtypes = [_C.POINTER(_C.c_void_p), _C.POINTER(Meta), _C.c_int, _C.POINTER(Reframe),
                                                   _C.POINTER(PixFormat), _C.c_int, _C.POINTER(RgbFormat), _C.POINTER(ResRung), _C.c_int,
                                                   _C.c_int, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_levels_identity.argtypes = [_C.POINTER(Levels)]
        L.dsv1_levels_range.argtypes = [_C.POINTER(Levels), _C.c_int, _C.c_int]
        L.dsv1_levels_adjust.argtypes = [_C.POINTER(Levels)] + [_C.c_int] * 5
        L.dsv1_levels_compose.argtypes = [_C.POINTER(Levels)] * 3
        L.dsv1_levels_is_identity.argtypes = [_C.POINTER(Levels)]
        L.dsv1_range_from_histogram.argtypes = [_C.c_void_p, _C.c_int, _C.c_int, _C.POINTER(_C.c_int)]
        L.dsv1_points_from_histogram.argtypes = [_C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.POINTER(_C.c_int), _C.POINTER(_C.c_int)]
        L.dsv1_levels_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.POINTER(Levels), _C.c_int]
        L.dsv1_histogram_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int]
        L.dsv1_detect_range_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.POINTER(_C.c_int), _C.c_int]
        L.dsv1_batch_set_source_levels.argtypes = [_C.c_void_p, _C.POINTER(Levels)]
        L.dsv1_resladder_set_levels.argtypes = [_C.c_void_p, _C.POINTER(Levels)]
        L.dsv1_overlay_bytes.restype = _C.c_size_t
        L.dsv1_overlay_bytes.argtypes = [_C.c_int] * 3
        L.dsv1_overlay_valid.argtypes = [_C.POINTER(Overlay)] + [_C.c_int] * 4
        L.dsv1_overlay_opacity_at.argtypes = [_C.POINTER(Overlay), _C.c_int64]
        L.dsv1_overlay_plan.restype = _C.c_longlong
        L.dsv1_overlay_plan.argtypes = [_C.POINTER(Overlay), _C.c_int, _C.c_int, _C.c_int, _C.POINTER(_C.c_int64), _C.c_int, _C.c_int, _C.c_int,
                                        _C.POINTER(OverlayItem), _C.c_longlong, _C.POINTER(_C.c_int)]
        L.dsv1_overlay_from_rgba.argtypes = [_C.c_void_p] + [_C.c_int] * 7 + [_C.c_void_p]
        L.dsv1_overlay_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.POINTER(Overlay), _C.c_int, _C.c_int64,
                                        _C.c_int]
        L.dsv1_batch_set_source_overlays.argtypes = [_C.c_void_p, _C.POINTER(Overlay), _C.c_int]
        L.dsv1_batch_overlay_seek.argtypes = [_C.c_void_p, _C.c_int, _C.c_int64]
        L.dsv1_resladder_set_overlays.argtypes = [_C.c_void_p, _C.POINTER(Overlay), _C.c_int]
        L.dsv1_resladder_overlay_seek.argtypes = [_C.c_void_p, _C.c_int, _C.c_int64]
        L.dsvg_dispatch_last.argtypes = [_C.POINTER(Dispatch)]
        L.dsvg_dispatch_plan.argtypes = [_C.c_int, _C.c_int, _C.c_int, _C.POINTER(Dispatch)]
        L.dsvg_inv_plan.argtypes = [_C.c_int] * 9 + [_C.c_uint, _C.c_int, _C.POINTER(InvStep), _C.c_int, _C.POINTER(_C.c_int)]
        L.dsv1_decbatch_set_draw_info.argtypes = [_C.c_void_p, _C.c_int]
        L.dsv1_packet_blockinfo.argtypes = [_C.c_void_p, _C.c_size_t, _C.c_int, _C.c_int, _C.POINTER(_C.c_int), _C.POINTER(_C.c_int),
                                            _C.POINTER(_C.c_int), _C.c_void_p, _C.c_size_t]
        L.dsv1_draw_info_clip.argtypes = [_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _C.c_void_p, _C.c_int,
                                          _C.c_int]
        L.dsv1_decbatch_set_output_scale.argtypes = [_C.c_void_p, _C.c_int, _C.c_int, _C.c_int]
        L.dsv1_decbatch_out_dims.argtypes = [_C.c_void_p, _C.POINTER(_C.c_int), _C.POINTER(_C.c_int)]
        L.dsvg_ctx_output_scale.argtypes = [_C.c_void_p, _C.c_int, _C.c_int, _C.c_int]
        _lib = L
    return _lib


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed rc=%d: %s" % (what, rc, lib().dsvg_last_error().decode()))


def dispatch_last():
    """what launch_fwd_sbt / launch_hme last decided in this process (dict, see Dispatch)"""
    d = Dispatch()
    _chk(lib().dsvg_dispatch_last(_C.byref(d)), "dsvg_dispatch_last")
    return d.as_dict()


def dispatch_plan(w, h, fmt):
    """what they decide for an encoder of this geometry; needs no device"""
    d = Dispatch()
    _chk(lib().dsvg_dispatch_plan(w, h, fmt, _C.byref(d)), "dsvg_dispatch_plan")
    return d.as_dict()


def inv_plan(w, h, fmt, group, isP, with_tail=1, insym=0, patch_kernel=0, fuse_border=0, switches=0, njobs=1):
    """the launches of launch_inv_sbt for plane group `group` (0 luma, 1 the chroma pair) of njobs pictures of an encoder of this
    geometry, with the A/B switches of the mask `switches` (INV_NO_*): ([step dicts in launch order], fb); needs no device"""
    steps, fb = (InvStep * 5)(), _C.c_int(0)
    n = lib().dsvg_inv_plan(w, h, fmt, group, isP, with_tail, insym, patch_kernel, fuse_border, switches, njobs, steps, 5, _C.byref(fb))
    if n < 0:
        _chk(n, "dsvg_inv_plan")
    return [steps[i].as_dict() for i in range(n)], fb.value


def fwd_plan(w, h, fmt, group, isP=0, general_whole=0, switches=0, njobs=1):
    """the forward launches of plane group `group` (0 luma, 1 the chroma pair) of njobs I or P pictures in the frame step of an encoder
    of this geometry, or (FWD_GROUP_STEP) what the step launches once for all planes, with the A/B switches of the mask `switches`
    (FWD_NO_*): ([step dicts in launch order], the DSVG_FWD_* mask or -1); needs no device"""
    L = lib()                                               # (bound here, not in lib(): an A/B build named by DSV1_SO may be older than this query)
    L.dsvg_fwd_plan.argtypes = [_C.c_int] * 6 + [_C.c_uint, _C.c_int, _C.POINTER(FwdStep), _C.c_int, _C.POINTER(_C.c_int)]
    steps, mask = (FwdStep * 5)(), _C.c_int(0)
    n = L.dsvg_fwd_plan(w, h, fmt, group, isP, general_whole, switches, njobs, steps, 5, _C.byref(mask))
    if n < 0:
        _chk(n, "dsvg_fwd_plan")
    return [steps[i].as_dict() for i in range(n)], mask.value


def hme_plan(w, h, fmt, npairs=1, csum_table=1):
    """the launches of the motion search of npairs pairs in an encoder of this geometry: [step dicts in launch order]; needs no device"""
    L = lib()
    L.dsvg_hme_plan.argtypes = [_C.c_int] * 5 + [_C.POINTER(HmeStep), _C.c_int]
    steps = (HmeStep * 14)()
    n = L.dsvg_hme_plan(w, h, fmt, csum_table, npairs, steps, 14)
    if n < 0:
        _chk(n, "dsvg_hme_plan")
    return [steps[i].as_dict() for i in range(n)]


def load_plan(w, h, fmt, pyramid_levels=0, with_pyramid=1, src_mod16=0, pitch_mod16=0, switches=0, n=1, n_chroma_in_place=0, n_luma_in_place=0):
    """what a source load of n frames decides in a context of this geometry (pyramid_levels as dsvg_ctx_create takes it), for a source at
    this address and frame distance modulo 16, with the A/B switches of the mask `switches` (LOAD_NO_*): a dict of dsvg_load_plan_out's fields, the
    bodies and kernels by name, `levels` a list of per-level dicts, `kernels` {kernel name: (launches, algorithmic bytes)} of the
    kernels that run; needs no device"""
    L = lib()
    L.dsvg_load_plan.argtypes = [_C.c_int] * 7 + [_C.c_uint, _C.c_int, _C.c_int, _C.c_int, _C.POINTER(LoadPlan)]
    p = LoadPlan()
    _chk(L.dsvg_load_plan(w, h, fmt, pyramid_levels, with_pyramid, src_mod16, pitch_mod16, switches, n, n_chroma_in_place, n_luma_in_place, _C.byref(p)), "dsvg_load_plan")
    d = {k: getattr(p, k) for k in ("sides", "fuse1", "fuse2", "sides1", "sides2", "grid_planes", "luma_sum", "luma_sum_dword", "ring_x16", "ring_y4",
                                    "chroma_in_place_ok", "luma_in_place_ok")}
    d["body"] = tuple(UNPACK_BODIES[b] for b in p.body)
    d["levels"] = []
    for l in range(p.levels + 1):
        o = p.level[l]
        lv = {k: getattr(o, k) for k in ("w", "h", "tb_only", "ds2x", "ds2x_sides", "ds2x_tail", "src_odd_w", "src_odd_h")}
        lv["border"] = BORDER_KERNELS[o.border]
        d["levels"].append(lv)
    d["kernels"] = {LOAD_KERNELS[k]: (p.launches[k], p.bytes[k]) for k in range(5) if p.launches[k]}
    return d


CTX_MEM_IDS = 84                                           # DSVG_CTX_MEM_IDS
MEM_KINDS = ("device", "pinned", "slab")


class CtxMemRow(_C.Structure):
    _fields_ = [("id", _C.c_int), ("kind", _C.c_int), ("zeroed", _C.c_int), ("count", _C.c_size_t), ("size", _C.c_size_t), ("pad", _C.c_size_t),
                ("bytes", _C.c_size_t)]


def _mem_lib():
    L = lib()
    geo = [_C.c_int] * 10
    L.dsvg_ctx_mem_name.restype = _C.c_char_p
    L.dsvg_ctx_mem_name.argtypes = [_C.c_int]
    L.dsvg_ctx_mem_plan.argtypes = geo + [_C.POINTER(CtxMemRow), _C.c_int, _C.POINTER(_C.c_size_t)]
    L.dsvg_ctx_mem_grow.restype = _C.c_size_t
    L.dsvg_ctx_mem_grow.argtypes = geo + [_C.c_int, _C.c_size_t, _C.c_size_t, _C.c_int]
    L.dsvg_ctx_mem_live.argtypes = [_C.c_void_p, _C.POINTER(_C.c_size_t), _C.c_int]
    L.dsvg_mem_outstanding.restype = None
    L.dsvg_mem_outstanding.argtypes = [_C.POINTER(_C.c_size_t)]
    L.dsvg_debug_fail_alloc_at.restype = None
    L.dsvg_debug_fail_alloc_at.argtypes = [_C.c_int]
    return L


def ctx_mem_names():
    """the short name of every buffer id of a context, creation-time and lazy, by id"""
    L = _mem_lib()
    return [L.dsvg_ctx_mem_name(i).decode() for i in range(CTX_MEM_IDS)]


def ctx_mem_plan(w, h, fmt, pyramid_levels=0, n_src_slots=1, n_recon_slots=1, max_jobs=1, out_slots=1, blk_w=0, blk_h=0):
    """the buffers dsvg_ctx_create_blk allocates for these arguments, in the order it allocates them: ([row dicts: id, name, kind, zeroed,
    count, size, pad, bytes], {"device": bytes, "pinned": bytes}); needs no device"""
    L = _mem_lib()
    rows, tot = (CtxMemRow * CTX_MEM_IDS)(), (_C.c_size_t * 2)()
    n = L.dsvg_ctx_mem_plan(w, h, fmt, pyramid_levels, n_src_slots, n_recon_slots, max_jobs, out_slots, blk_w, blk_h, rows, CTX_MEM_IDS, tot)
    if n < 0:
        _chk(n, "dsvg_ctx_mem_plan")
    names = ctx_mem_names()
    return ([{"id": r.id, "name": names[r.id], "kind": MEM_KINDS[r.kind], "zeroed": bool(r.zeroed), "count": r.count, "size": r.size, "pad": r.pad,
              "bytes": r.bytes} for r in rows[:n]], {"device": tot[0], "pinned": tot[1]})


def ctx_mem_grow(name, need, cap, few=False, **geo):
    """the bytes the lazy buffer `name` takes when it holds `cap` elements and `need` are asked for, in a context of the arguments `geo` (those
    of ctx_mem_plan: w, h, fmt, ...); needs no device"""
    a = dict(pyramid_levels=0, n_src_slots=1, n_recon_slots=1, max_jobs=1, out_slots=1, blk_w=0, blk_h=0)
    a.update(geo)
    return int(_mem_lib().dsvg_ctx_mem_grow(a["w"], a["h"], a["fmt"], a["pyramid_levels"], a["n_src_slots"], a["n_recon_slots"], a["max_jobs"], a["out_slots"],
                                            a["blk_w"], a["blk_h"], ctx_mem_names().index(name), need, cap, 1 if few else 0))


def ctx_mem_live(ctx):
    """{buffer name: bytes} the device context `ctx` holds now (every id; 0: not allocated)"""
    b = (_C.c_size_t * CTX_MEM_IDS)()
    _chk(_mem_lib().dsvg_ctx_mem_live(ctx, b, CTX_MEM_IDS), "dsvg_ctx_mem_live")
    return dict(zip(ctx_mem_names(), (int(v) for v in b)))


def mem_outstanding():
    """(device bytes, pinned bytes) held by all live contexts of the process"""
    o = (_C.c_size_t * 2)()
    _mem_lib().dsvg_mem_outstanding(o)
    return int(o[0]), int(o[1])


def code_batch_plan(w, h, fmt, n_recon_slots, n_src_slots, max_jobs, out_slots, code_streams, switches, nsteps, njobs, jobs, rc=None):
    """what dsvg_code_batch (rc: dsvg_code_batch_rc) decides on the host for `jobs` (a ctypes array of PicJob, jobs[step * njobs + j]; rc
    one of RcJob) in an encoder context created with these arguments, with the A/B switches of the mask `switches` (BATCH_*): a dict of
    dsvg_batch_plan's fields, the arrays as numpy arrays cut to their lengths (ext: [total, 8]; the per-share ones: [nsteps, ng]).
    Raises BatchRefused with the call's own code and text for jobs the call refuses.  Needs no device"""
    total = max(nsteps * njobs, 1)
    d = Dispatch()                                          # (the block size of the geometry: how long the intra list can get)
    nblk = -(-w // d.blk_w) * -(-h // d.blk_h) if lib().dsvg_dispatch_plan(w, h, fmt, _C.byref(d)) == 0 else 1
    groups = max(nsteps, 1) * 4
    arr = {"nI": _np.zeros(max(nsteps, 1), _np.int32), "order": _np.zeros(total, _np.int32), "mvu": _np.zeros(total, _np.int32),
           "stu": _np.zeros(total, _np.int32), "mvcp": _np.zeros(total, _np.uint8), "stcp": _np.zeros(total, _np.uint8),
           "ext": _np.zeros(total * 8, _np.int16), "rc_next": _np.zeros(total, _np.int32), "ioff": _np.zeros(groups, _np.int32),
           "icnt": _np.zeros(groups, _np.int32), "noint": _np.zeros(groups, _np.uint8), "keeps": _np.zeros(groups, _np.uint8),
           "ilist": _np.zeros(total * nblk, _np.int32)}
    p = BatchPlan(cap_steps=len(arr["nI"]), cap_jobs=total, cap_groups=groups, cap_ilist=total * nblk)
    for k, a in arr.items():
        setattr(p, k, a.ctypes.data)
    # (bound here, not in lib(): an A/B build named by DSV1_SO may be older than this query)
    lib().dsvg_code_batch_plan.argtypes = [_C.c_int] * 8 + [_C.c_uint, _C.c_int, _C.c_int, _C.POINTER(PicJob), _C.POINTER(RcJob), _C.POINTER(BatchPlan)]
    r = lib().dsvg_code_batch_plan(w, h, fmt, n_recon_slots, n_src_slots, max_jobs, out_slots, code_streams, switches, nsteps, njobs, jobs, rc,
                                   _C.byref(p))
    if r != 0:
        raise BatchRefused(r, lib().dsvg_last_error().decode())
    d = {k: getattr(p, k) for k in ("nblk", "mc_fused", "base", "total", "ng", "iln", "nmv", "nst", "mv_contig", "par_enqueue")}
    d["gk"] = tuple(p.gk)[:p.ng + 1]
    for k in ("order", "mvu", "stu", "mvcp", "stcp", "rc_next"):
        d[k] = arr[k][:p.total]
    d["nI"] = arr["nI"][:nsteps]
    d["ext"] = arr["ext"][:p.total * 8].reshape(p.total, 8)
    for k in ("ioff", "icnt", "noint", "keeps"):
        d[k] = arr[k][:nsteps * p.ng].reshape(nsteps, p.ng)
    d["ilist"] = arr["ilist"][:p.iln]
    return d


def decode_plan(w, h, fmt, n_recon_slots, max_jobs, switches, force32, draw_mode, njobs, jobs):
    """what dsvg_decode_pictures decides on the host for `jobs` (a ctypes array of DecJob) in a context created with these arguments,
    with the A/B switches of the mask `switches` (DEC_*): a dict of dsvg_dec_plan's fields, the arrays as numpy arrays cut to their
    lengths (the per-plane ones: [njobs, 3]; lim: [2, 16]).  Raises DecodeRefused with the call's own code and text for jobs the call
    refuses.  Needs no device"""
    n = max(njobs, 1)
    d = Dispatch()                                          # (the block size of the geometry: how long the list can get)
    nblk = -(-w // d.blk_w) * -(-h // d.blk_h) if lib().dsvg_dispatch_plan(w, h, fmt, _C.byref(d)) == 0 else 1
    arr = {"order": _np.zeros(n, _np.int32), "path": _np.zeros(n, _np.int32), "dec_sym": _np.zeros(3 * n, _np.int32),
           "wide": _np.zeros(n, _np.uint8), "inplace": _np.zeros(n, _np.uint8), "dc": _np.zeros(3 * n, _np.int32),
           "runs": _np.zeros(3 * n, _np.int32), "len": _np.zeros(3 * n, _np.int32), "bitpos": _np.zeros(3 * n, _np.int64),
           "blob_off": _np.zeros(3 * n, _np.int64), "meta_off": _np.zeros(3 * n, _np.int64), "ilist": _np.zeros(n * nblk, _np.int32)}
    p = DecPlan(cap_jobs=n, cap_ilist=n * nblk)
    for k, a in arr.items():
        setattr(p, k, a.ctypes.data)
    lib().dsvg_decode_plan.argtypes = [_C.c_int] * 5 + [_C.c_uint, _C.c_int, _C.c_int, _C.c_int, _C.POINTER(DecJob), _C.POINTER(DecPlan)]
    r = lib().dsvg_decode_plan(w, h, fmt, n_recon_slots, max_jobs, switches, int(force32), draw_mode, njobs, jobs, _C.byref(p))
    if r != 0:
        raise DecodeRefused(r, lib().dsvg_last_error().decode())
    out = {k: getattr(p, k) for k in ("nblk", "nbh", "mc_patch", "second_stream", "nI", "blob", "nmeta", "max_entries", "max_chunks", "insym", "f0",
                                      "anysym", "scatter_one", "resolve", "fork", "mc", "ex0", "ey0", "iln", "draw0", "draw1")}
    out["sym_ok"], out["ov"], out["nchunks"] = tuple(p.sym_ok), tuple(p.ov), tuple(p.nchunks)
    out["lim"] = _np.array([list(p.lim[0]), list(p.lim[1])], dtype=_np.int64)
    for k in ("order", "path", "wide", "inplace"):
        out[k] = arr[k][:njobs]
    for k in ("dec_sym", "dc", "runs", "len", "bitpos", "blob_off", "meta_off"):
        out[k] = arr[k][:3 * njobs].reshape(njobs, 3)
    out["ilist"] = arr["ilist"][:p.iln]
    return out


FETCH_NO_FAST = 1                                          # DSVG_FETCH_*


class FetchPlan(_C.Structure):
    """dsvg_fetch_plan_out (include/dsvg.h): the plan of a packet fetch, arrays of the caller's"""
    _fields_ = [("cap_pics", _C.c_int), ("cap_pieces", _C.c_int), ("wait", _C.c_void_p), ("copies", _C.c_void_p), ("rows", _C.c_void_p),
                ("nbytes", _C.c_void_p), ("pay", _C.c_void_p), ("piece", _C.c_void_p), ("piece_bytes", _C.c_void_p),
                ("few", _C.c_int), ("stream_wait", _C.c_int), ("nwait", _C.c_int), ("lo", _C.c_int), ("hi", _C.c_int), ("fits", _C.c_int),
                ("general", _C.c_int), ("nchunks", _C.c_int), ("grow_few", _C.c_ulonglong), ("total", _C.c_ulonglong), ("grow", _C.c_ulonglong)]


class FetchRefused(RuntimeError):
    """dsvg_fetch_plan did not answer with a plan: rc and text are what the fetch itself would return and set; grow_few, grow: what the
    call had asked of its payload pair by then"""
    def __init__(self, rc, text, grow_few=0, grow=0):
        super().__init__("dsvg_fetch_plan failed rc=%d: %s" % (rc, text))
        self.rc, self.text, self.grow_few, self.grow = rc, text, grow_few, grow


def fetch_plan(ctx_out_slots, out_slots, slot_ev, slot_isP, nring, ncalls, has_cb, switches, bits_per_job, bits_off, bits_cap, total_bits, overflow,
               nchunks=1, align=1):
    """what dsvg_fetch_pictures_cb decides on the host for the out slots `out_slots` of a context with `ctx_out_slots` of them, whose
    slots were coded last by the events slot_ev (indices into a ring of nring, -1: never) and hold P pictures where slot_isP says so
    (may be short or empty), after ncalls coding calls, with the A/B switches of the mask `switches` (FETCH_*) and the plane summaries
    total_bits / overflow ([n, 3]) as they come back: a dict of dsvg_fetch_plan_out's fields, the arrays as numpy arrays cut to their
    lengths (copies, rows: [n, 3, 3]; nbytes, pay: [n, 3]; pieces: [(first, end, o0, o1)]).  Raises FetchRefused with the call's own
    code and text.  Needs no device"""
    n = len(out_slots)
    m = max(n, 1)
    arr = {"wait": _np.zeros(m, _np.int32), "copies": _np.zeros(9 * m, _np.uint64), "rows": _np.zeros(9 * m, _np.uint64),
           "nbytes": _np.zeros(3 * m, _np.uint32), "pay": _np.zeros(3 * m, _np.uint64), "piece": _np.zeros(2 * max(nchunks, 1), _np.int32),
           "piece_bytes": _np.zeros(2 * max(nchunks, 1), _np.uint64)}
    p = FetchPlan(cap_pics=m, cap_pieces=max(nchunks, 1))
    for k, a in arr.items():
        setattr(p, k, a.ctypes.data)
    slots = (_C.c_int * m)(*out_slots)
    ev = (_C.c_int * max(len(slot_ev), 1))(*slot_ev)
    isp = (_C.c_ubyte * max(len(slot_isP), 1))(*slot_isP)
    bits = (_C.c_ulonglong * 7)(bits_per_job, *bits_off, *bits_cap)
    tb = _np.ascontiguousarray(_np.asarray(total_bits, _np.uint64).reshape(-1))
    ov = _np.ascontiguousarray(_np.asarray(overflow, _np.int32).reshape(-1))
    assert len(tb) >= 3 * n and len(ov) >= 3 * n and len(slot_ev) >= ctx_out_slots
    f = lib().dsvg_fetch_plan
    f.argtypes = [_C.c_int, _C.c_int, _C.POINTER(_C.c_int), _C.POINTER(_C.c_int), _C.c_int, _C.POINTER(_C.c_ubyte), _C.c_int, _C.c_longlong, _C.c_int,
                  _C.c_uint, _C.POINTER(_C.c_ulonglong), _C.c_void_p, _C.c_void_p, _C.c_int, _C.c_int, _C.POINTER(FetchPlan)]
    r = f(ctx_out_slots, n, slots, ev, len(slot_isP), isp, nring, ncalls, int(bool(has_cb)), switches, bits, tb.ctypes.data, ov.ctypes.data,
          nchunks, align, _C.byref(p))
    if r != 0:
        raise FetchRefused(r, lib().dsvg_last_error().decode(), p.grow_few, p.grow)
    d = {k: getattr(p, k) for k in ("few", "stream_wait", "lo", "hi", "fits", "general", "nchunks", "grow_few", "total", "grow")}
    d["wait"] = arr["wait"][:p.nwait].tolist()
    d["copies"] = arr["copies"][:9 * n * p.few].reshape(-1, 3, 3)
    d["rows"] = arr["rows"][:9 * n * p.general].reshape(-1, 3, 3)
    d["nbytes"], d["pay"] = arr["nbytes"][:3 * n].reshape(n, 3), arr["pay"][:3 * n].reshape(n, 3)
    d["pieces"] = [(int(arr["piece"][2 * j]), int(arr["piece"][2 * j + 1]), int(arr["piece_bytes"][2 * j]), int(arr["piece_bytes"][2 * j + 1]))
                   for j in range(p.nchunks)]
    return d


def make_encoder_cfg(w, h, fmt, qp=85, gop=12, rc_mode_cli=1, kbps=0, scd=1, ipct=50, pyrlevels=0, stabref=0,
                     fps_num=30, fps_den=1):
    """fill a DSV_ENCODER exactly like the reference CLI does for these flags (dsv_main.c:423-489):
    rc_mode_cli 0 = ABR, 1 = CRF (CLI numbering); kbps 0 = auto; stabref 0 = auto"""
    L = lib()
    e = Encoder()
    L.dsv_enc_init(_C.byref(e))
    e.vidmeta = Meta(w, h, fmt, fps_num, fps_den, 1, 1)
    e.gop = gop
    e.scene_change_delta = 4
    e.do_scd = scd
    e.intra_pct_thresh = ipct
    e.quality = MAX_QUALITY * qp // 100
    e.rc_mode = 0 if rc_mode_cli == 1 else 1
    e.bitrate = kbps * 1024 if kbps else L.estimate_bitrate(e.quality * 100 // MAX_QUALITY, gop, _C.byref(e.vidmeta))
    if e.rc_mode == 1:
        e.quality = min(max(e.quality * 3 // 2, 0), MAX_QUALITY)
    e.max_q_step = MAX_QUALITY // 200
    e.min_quality = MAX_QUALITY * 1 // 100
    e.max_quality = MAX_QUALITY
    e.min_I_frame_quality = MAX_QUALITY * 5 // 100
    e.rc_high_motion_nudge = 1
    e.pyramid_levels = pyrlevels
    e.stable_refresh = stabref if stabref else min(max(gop - 1, 1), 14)
    return e


def _take(buf):
    data = _C.string_at(buf.data, buf.len) if buf.len else b""
    if buf.data:
        lib().dsv_free(_C.cast(buf.data, _C.c_void_p))
    return data


class StreamBytes:
    """The finished packets of one stream exactly where the library assembled them (a dsv_alloc'd host buffer): no copy
    into a Python bytes object.  len(), bytes(), memoryview() work; the buffer is freed with the object."""

    def __init__(self, buf):
        self._ptr = _C.cast(buf.data, _C.c_void_p).value
        self._len = int(buf.len) if self._ptr else 0

    def __len__(self):
        return self._len

    def __bytes__(self):
        return _C.string_at(self._ptr, self._len) if self._len else b""

    def view(self):
        return memoryview((_C.c_ubyte * self._len).from_address(self._ptr)) if self._len else memoryview(b"")

    def __eq__(self, other):
        return bytes(self) == bytes(other)

    def __del__(self):
        if getattr(self, "_ptr", None):
            try:
                lib().dsv_free(_C.c_void_p(self._ptr))
            except Exception:      # interpreter shutdown
                pass
            self._ptr = None


class Batch:
    """nstreams independent encoder streams, frames_per_call frames each per encode() call"""

    def __init__(self, cfg, nstreams, frames_per_call, device=0, chains=0):
        """chains > 0: ONE stream in chain mode (dsv1_stream_open): frames_per_call consecutive frames per call, the chains of
        pictures between I pictures coded side by side"""
        self.L = lib()
        self.h = _C.c_void_p(None)
        self.nstreams, self.F = nstreams, frames_per_call
        self.nsources = nstreams                 # (input frames come per source: a Ladder has fewer sources than output streams)
        if chains:
            assert nstreams == 1
            _chk(self.L.dsv1_stream_open(_C.byref(self.h), _C.byref(cfg), device, frames_per_call, chains), "dsv1_stream_open")
        else:
            _chk(self.L.dsv1_batch_open(_C.byref(self.h), _C.byref(cfg), device, nstreams, frames_per_call), "dsv1_batch_open")
        self._opened(cfg)

    def _opened(self, cfg):
        self.ctx = self.L.dsv1_batch_ctx(self.h)
        m = cfg.vidmeta
        self.width, self.height, self.fmt = m.width, m.height, m.subsamp
        self._dev = []
        self._pin = []

    def mem_live(self):
        """{buffer name: bytes} the batch's device context holds now (ctx_mem_live)"""
        return ctx_mem_live(self.ctx)

    def _input(self, yuv):
        """a host clip as the C entry points read it: nsources x F frames, whatever it is given (checked here)"""
        a = _np.ascontiguousarray(yuv, dtype=_np.uint8)
        fin = self.in_frames
        if a.size != self.nsources * fin * self.frame_bytes:
            raise ValueError("a batch is %d %s x %d frames x %d bytes, got %d bytes" % (
                self.nsources, "streams" if self.nsources == self.nstreams else "sources", fin, self.frame_bytes, a.size))
        return a

    _SOURCE_INPUT = "dsv1_batch_source_input"

    def _source_input(self):
        """(frames per source and call, bytes per frame, (width, height) of the raw picture) a call must bring, straight from the
        session's source chain (dsv1_batch_source_input, dsv1_resladder_source_input): nothing of it is kept here"""
        v, fb = (_C.c_int * 3)(), _C.c_size_t()
        _chk(getattr(self.L, self._SOURCE_INPUT)(self.h, v, _C.byref(fb)), self._SOURCE_INPUT)
        return v[0], fb.value, (v[1], v[2])

    @property
    def in_frames(self):
        """input frames per source and call: frames_per_call, half of it behind a field-rate deinterlacer, 5/4 of it in front of the
        inverse telecine"""
        return self._source_input()[0] if getattr(self, "h", None) else self.F

    @property
    def frame_bytes(self):
        """bytes from frame to frame of the clips that come in: the source format's, at in_dims"""
        return self._source_input()[1] if getattr(self, "h", None) else self._frame_bytes

    @frame_bytes.setter
    def frame_bytes(self, n):
        self._frame_bytes = n                   # (an object without a session: the tests of the length check build one)

    def set_source_ivtc(self, iv):
        """from the next submit on the clips are 3:2 pulled-down film and inverse telecined on the GPU as Ivtc iv says, behind the source
        format's conversion, in the deinterlacer's place and exclusive with it (dsv1_batch_set_source_ivtc); None switches it off.
        Between batches only; forgets every source's state.  frames_per_call counts coded pictures and must be a multiple of 4: a call
        takes in_frames = 5 * frames_per_call / 4 frames per source."""
        _chk(self.L.dsv1_batch_set_source_ivtc(self.h, _C.byref(iv) if iv is not None else None), "dsv1_batch_set_source_ivtc")

    def ivtc_reset(self, source=-1):
        """a discontinuity: the next frame of `source` (-1: every source) is a stream's first picture (dsv1_batch_ivtc_reset)"""
        _chk(self.L.dsv1_batch_ivtc_reset(self.h, source), "dsv1_batch_ivtc_reset")

    def set_source_deinterlace(self, di):
        """from the next submit on the clips are interlaced and deinterlaced on the GPU as Deint di says, behind the source format's
        conversion (dsv1_batch_set_source_deinterlace); None switches it off.  Between batches only; forgets every source's history.
        frames_per_call counts coded pictures: with DEINT_FIELD a call takes in_frames = frames_per_call / 2 frames per source."""
        _chk(self.L.dsv1_batch_set_source_deinterlace(self.h, _C.byref(di) if di is not None else None), "dsv1_batch_set_source_deinterlace")

    def deinterlace_reset(self, source=-1):
        """a discontinuity: the next frame of `source` (-1: every source) is deinterlaced as a stream's first (dsv1_batch_deinterlace_reset)"""
        _chk(self.L.dsv1_batch_deinterlace_reset(self.h, source), "dsv1_batch_deinterlace_reset")

    def set_source_denoise(self, dn):
        """from the next submit on the clips pass the temporal noise filter on the GPU as Denoise dn says, behind the source format's
        conversion and the deinterlacer (dsv1_batch_set_source_denoise); None switches it off.  Between batches only; forgets every
        source's filter state."""
        _chk(self.L.dsv1_batch_set_source_denoise(self.h, _C.byref(dn) if dn is not None else None), "dsv1_batch_set_source_denoise")

    def denoise_reset(self, source=-1):
        """a discontinuity: the next picture of `source` (-1: every source) is filtered as a stream's first (dsv1_batch_denoise_reset)"""
        _chk(self.L.dsv1_batch_denoise_reset(self.h, source), "dsv1_batch_denoise_reset")

    def set_source_levels(self, lv):
        """from the next submit on the clips pass Levels lv on the GPU (dsv1_batch_set_source_levels), directly behind the source format's
        conversion and in front of the deinterlacer or the inverse telecine; None or the identity switches it off.  Set AFTER a reframe
        and an orientation.  Between batches only; forgets the deinterlacer's history, the inverse telecine's and the noise filter's
        state of every source."""
        _chk(self.L.dsv1_batch_set_source_levels(self.h, _C.byref(lv) if lv is not None else None), "dsv1_batch_set_source_levels")

    def set_source_overlays(self, overlays):
        """from the next submit on the Overlay objects of the list are blended onto the clips on the GPU, in list order, as the LAST
        source pass (dsv1_batch_set_source_overlays); None or an empty list switches it off.  The bitmaps are copied.  Every source's
        picture counter starts at 0 and advances by frames_per_call per call.  Only with nothing in flight and nothing staged; one
        invalid item refuses the list and leaves the setting as it was."""
        arr, n = _overlay_array(overlays)
        _chk(self.L.dsv1_batch_set_source_overlays(self.h, arr, n), "dsv1_batch_set_source_overlays")

    def overlay_seek(self, source, t):
        """the next picture of `source` (-1: every source) is picture t of the overlays' clock (dsv1_batch_overlay_seek)"""
        _chk(self.L.dsv1_batch_overlay_seek(self.h, source, t), "dsv1_batch_overlay_seek")

    def set_source_reframe(self, rf):
        """from the next submit on the clips are rf.in_w x rf.in_h and reframed on the GPU onto the batch's geometry as Reframe rf says,
        as the LAST source pass (dsv1_batch_set_source_reframe); None, or the identity, switches it off.  Only with nothing in flight
        and no source format, RGB format, deinterlacer or noise filter set: those are set AFTER it and resolve at the input geometry.
        The input-length check follows."""
        _chk(self.L.dsv1_batch_set_source_reframe(self.h, _C.byref(rf) if rf is not None else None), "dsv1_batch_set_source_reframe")

    def set_source_orient(self, orient):
        """from the next submit on the clips are oriented on the GPU by code `orient` (Orient.*; dsv1_batch_set_source_orient) behind
        the noise filter and in front of the reframe; 0 switches it off.  The oriented picture is the reframe's input (set BEFORE
        this) or the batch's geometry; the clips come in at the raw geometry, orient_dims(orient_inverse(orient), ...) of it.  Only
        with nothing in flight and no source format, RGB format, deinterlacer, inverse telecine or noise filter set: those are set
        AFTER it and resolve at the raw geometry.  The input-length check follows."""
        _chk(self.L.dsv1_batch_set_source_orient(self.h, orient), "dsv1_batch_set_source_orient")

    @property
    def in_dims(self):
        """(width, height) of the frames that come in: the batch's geometry, or the input of the reframe set, turned back by the
        orientation set"""
        return self._source_input()[2]

    def set_fnum(self, stream, fnum):
        self.L.dsv1_batch_set_fnum(self.h, stream, fnum)

    def set_source_format(self, pf, src_subsamp=None):
        """from the next submit on, encode() / submit() take clips of PixFormat pf (dsv1_batch_set_source_format), converted on the
        GPU; None switches back to packed planar 8-bit.  Between batches only.  The input-length check follows the format.
        src_subsamp: the clips' subsampling where it is not the batch's (dsv1_batch_set_source_format_sub) -- 4:4:4 or 4:2:2, chroma
        halved on the way; pf None then means packed planar 8-bit at src_subsamp."""
        if src_subsamp is None:
            _chk(self.L.dsv1_batch_set_source_format(self.h, _C.byref(pf) if pf is not None else None), "dsv1_batch_set_source_format")
        else:
            _chk(self.L.dsv1_batch_set_source_format_sub(self.h, _C.byref(pf) if pf is not None else None, src_subsamp),
                 "dsv1_batch_set_source_format_sub")

    def set_source_rgb(self, rf):
        """from the next submit on, encode() / submit() take RGB clips of RgbFormat rf (dsv1_batch_set_source_rgb), converted on the
        GPU to the batch's subsampling; None switches back to packed planar 8-bit.  Between batches only; replaces a source format
        set before.  The input-length check follows."""
        _chk(self.L.dsv1_batch_set_source_rgb(self.h, _C.byref(rf) if rf is not None else None), "dsv1_batch_set_source_rgb")

    def set_source_hdr(self, pf, tables, src_subsamp=None, upsample=CHROMA_LINEAR):
        """from the next submit on, encode() / submit() take HDR clips of PixFormat pf (depth 10, 12 or 16) at src_subsamp (None: the
        batch's), tone-mapped to SDR on the GPU by HdrTables `tables` (dsv1_batch_set_source_hdr); tables None switches back to packed
        planar 8-bit.  Between batches only; replaces a source format or RGB format set before.  The input-length check follows."""
        _chk(self.L.dsv1_batch_set_source_hdr(self.h, _C.byref(pf) if pf is not None else None, self.fmt if src_subsamp is None else src_subsamp,
                                              _C.byref(tables) if tables is not None else None, upsample), "dsv1_batch_set_source_hdr")

    def dropped_recons(self):
        """(dropped, remedied): reference pictures coded without a reconstruction because nobody predicts from them / coded again
        because a renumbered stream did after all (include/dsv1_api.h, dsv1_batch_dropped_recons)"""
        r = _C.c_long(0)
        n = self.L.dsv1_batch_dropped_recons(self.h, _C.byref(r))
        return int(n), int(r.value)

    def recon_all(self, on=True):
        """reconstruct every reference picture (on) / drop the ones nobody predicts from (off, the default); between batches"""
        _chk(self.L.dsv1_batch_recon_all(self.h, 1 if on else 0), "dsv1_batch_recon_all")

    def sse_enable(self, on=True):
        """measure the pictures of the batches submitted from now on (on) / stop measuring (off); between batches only.
        The packets are the same either way (include/dsv1_api.h, dsv1_batch_sse_enable)"""
        _chk(self.L.dsv1_batch_sse_enable(self.h, 1 if on else 0), "dsv1_batch_sse_enable")

    def sse(self):
        """the batch collected last: per stream, frame (submitted order) and plane Y, U, V the exact sum of squared errors
        source vs reconstruction over the picture area -> numpy.uint64 [nstreams, F, 3].  Raises if it was not measured."""
        return _figures(self.L.dsv1_batch_get_sse, self.h, (self.nstreams, self.F, 3), _np.uint64)

    def psnr(self):
        """the same as PSNR in dB, float64 [nstreams, F, 4]: planes Y, U, V, then the whole picture (inf where SSE is 0)"""
        return psnr_db(self.sse(), self.width, self.height, self.fmt)

    def ssim_enable(self, on=True):
        """measure the SSIM of the pictures of the batches submitted from now on (on) / stop (off); between batches only, independent
        of sse_enable.  The packets are the same either way (include/dsv1_api.h, dsv1_batch_ssim_enable)"""
        _chk(self.L.dsv1_batch_ssim_enable(self.h, 1 if on else 0), "dsv1_batch_ssim_enable")

    def ssim_fx(self):
        """the batch collected last: per stream, frame (submitted order) and plane Y, U, V the exact fixed-point SSIM -- the sum over
        the plane's 8x8 windows at stride 4 of rint(2^32 SSIM) -> numpy.int64 [nstreams, F, 3].  Raises if it was not measured."""
        return _figures(self.L.dsv1_batch_get_ssim, self.h, (self.nstreams, self.F, 3), _np.int64)

    def ssim(self):
        """the same as mean SSIM, float64 [nstreams, F, 4]: planes Y, U, V, then the whole picture (weighted by window count)"""
        return ssim_mean(self.ssim_fx(), self.width, self.height, self.fmt)

    def encoder(self, stream):
        """the stream's DSV_ENCODER (owned by the batch): its public parameter fields may be changed between submits"""
        p = self.L.dsv1_batch_encoder(self.h, stream)
        if not p:
            raise IndexError("no stream %d" % stream)
        return Encoder.from_address(p)

    def upload(self, clip):
        """keep a raw clip (numpy uint8, any shape) resident in HBM; returns the device pointer"""
        a = _np.ascontiguousarray(clip, dtype=_np.uint8)
        p = _C.c_void_p(None)
        _chk(self.L.dsvg_dev_alloc(self.ctx, _C.byref(p), a.nbytes), "dsvg_dev_alloc")
        _chk(self.L.dsvg_dev_upload(self.ctx, p, a.ctypes.data, a.nbytes), "dsvg_dev_upload")
        self._dev.append(p)
        return p

    def pinned(self, shape):
        """uint8 numpy array in pinned host memory (dsvg_host_alloc): uploads from it are asynchronous"""
        n = int(_np.prod(shape))
        p = _C.c_void_p(None)
        _chk(self.L.dsvg_host_alloc(self.ctx, _C.byref(p), n), "dsvg_host_alloc")
        self._pin.append(p)
        return _np.ctypeslib.as_array(_C.cast(p, _C.POINTER(_C.c_uint8)), shape=(n,)).reshape(shape)

    def stage(self, yuv):
        """queue the upload of the host clip of a coming submit() (up to two; submit() must get the same memory)"""
        assert yuv.dtype == _np.uint8 and yuv.flags["C_CONTIGUOUS"]
        self._keep_staged = (getattr(self, "_keep_staged", []) + [yuv])[-3:]
        _chk(self.L.dsv1_batch_stage(self.h, yuv.ctypes.data), "dsv1_batch_stage")

    def encode(self, yuv, on_device=False, eos=False):
        """yuv: numpy [nstreams][F][frame_bytes] (host) or a device pointer from upload();
        returns one bytes object per stream"""
        bufs = (Buf * self.nstreams)()
        if on_device:
            ptr = yuv
        else:
            a = self._input(yuv)
            ptr = a.ctypes.data
        _chk(self.L.dsv1_batch_encode(self.h, ptr, 1 if on_device else 0, bufs), "dsv1_batch_encode")
        if eos:
            for s in range(self.nstreams):
                _chk(self.L.dsv1_batch_eos(self.h, s, _C.byref(bufs[s])), "dsv1_batch_eos")
        return [_take(bufs[s]) for s in range(self.nstreams)]

    def submit(self, yuv, on_device=False, held=False):
        """pipelined form: enqueue one batch (returns while its residual coding still runs on the GPU).
        At most two batches may be in flight: steady state is submit(i+1); collect(i).
        Device clips: by default (the contract of dsv1_api.h's plain yuv_on_device = 1) the clip is copied whole and may change
        as soon as submit() returns; held=True (DSV1_CLIP_HELD, what bench.py times): the caller keeps the clip unchanged until
        collect() of this batch returned -- its chroma is then read in place"""
        if on_device:
            ptr = yuv
        else:
            self._keep = self._input(yuv)
            ptr = self._keep.ctypes.data
        if not hasattr(self, "_abr"):
            self._abr = []
        bufs = (Buf * self.nstreams)()
        _chk(self.L.dsv1_batch_submit(self.h, ptr, (2 if held else 1) if on_device else 0, bufs), "dsv1_batch_submit")
        self._abr.append(bufs)

    def collect(self, copy=True):
        """fetch + assemble the oldest submitted batch -> one bytes object per stream (copy=False: StreamBytes
        objects that keep the packets in the buffers the library assembled them in)"""
        bufs = self._abr.pop(0)
        _chk(self.L.dsv1_batch_collect(self.h, bufs), "dsv1_batch_collect")
        if not copy:
            return [StreamBytes(bufs[s]) for s in range(self.nstreams)]
        return [_take(bufs[s]) for s in range(self.nstreams)]

    def sync(self):
        _chk(self.L.dsvg_ctx_sync(self.ctx), "dsvg_ctx_sync")

    def code_streams(self, n=0):
        """set (n >= 1) / query (n = 0) the number of coding streams; returns the previous value"""
        return self.L.dsvg_ctx_code_streams(self.ctx, n)

    def tile_stats(self, enable=True):
        """inverse-transform tiles of P pictures since the previous call: dict general_luma / general_chroma (computed)
        and zero_luma / zero_chroma (found empty: reconstruction = prediction); counting continues only if `enable`.
        Syncs and clears the counters."""
        v = (_C.c_ulonglong * 8)()
        _chk(self.L.dsvg_ctx_tile_stats2(self.ctx, v, 1 if enable else 0), "dsvg_ctx_tile_stats2")
        return {"general_luma": v[0], "general_chroma": v[1], "zero_luma": v[2], "zero_chroma": v[3],
                "flagged_patches_luma": v[4], "flagged_patches_chroma": v[5], "moved_unflagged_patches_chroma": v[6],
                "fused_border_bytes": v[7]}

    def kernel_names(self):
        return [self.L.dsvg_prof_kernel_name(i).decode() for i in range(self.L.dsvg_prof_kernels())]

    def mark(self, which):
        """HIP-event mark on the first coding stream (0: a timed region starts, 1: behind its last enqueued coding work)"""
        _chk(self.L.dsvg_ctx_mark(self.ctx, which), "dsvg_ctx_mark")

    def mark_ms(self):
        ms = _C.c_float(0)
        _chk(self.L.dsvg_ctx_mark_ms(self.ctx, _C.byref(ms)), "dsvg_ctx_mark_ms")
        return ms.value

    def breakdown_start(self):
        """start the per-step accounting of a timed loop: host phases of submit / collect (process-wide), the fetch's host side and the
        device-side marks of the pipeline's streams (dsvg_ctx_timeline)"""
        self.L.dsv1_host_prof_enable(1)
        v = (_C.c_double * 5)()
        _chk(self.L.dsvg_ctx_fetch_prof(self.ctx, v, 1), "dsvg_ctx_fetch_prof")
        _chk(self.L.dsvg_ctx_timeline(self.ctx, 1), "dsvg_ctx_timeline")

    def breakdown_stop(self, steps):
        """-> dict of ms per step (call after sync()): where the host thread spent a step, what the pipeline's streams did meanwhile"""
        n = self.L.dsv1_host_prof_get(None, 0, None)
        ms = (_C.c_double * n)()
        nb = _C.c_long(0)
        self.L.dsv1_host_prof_get(ms, n, _C.byref(nb))
        f = (_C.c_double * 5)()
        _chk(self.L.dsvg_ctx_fetch_prof(self.ctx, f, 1), "dsvg_ctx_fetch_prof")
        t = (_C.c_double * 12)()
        _chk(self.L.dsvg_ctx_timeline_get(self.ctx, t), "dsvg_ctx_timeline_get")
        _chk(self.L.dsvg_ctx_timeline(self.ctx, 0), "dsvg_ctx_timeline")
        self.L.dsv1_host_prof_enable(0)
        k = float(max(steps, 1))
        host = {self.L.dsv1_host_prof_name(i).decode(): round(ms[i], 3) for i in range(n)}
        nph = max(t[0], 1.0)
        return {"host_ms_per_batch": host, "host_batches": int(nb.value),
                "fetch_host_ms_per_call": {"wait_for_coding": round(f[0], 3), "sizes_round_trip": round(f[1], 3), "gather_copy_assembly": round(f[2], 3)},
                "fetch_bytes_per_call": int(f[3]), "fetch_calls": int(f[4]),
                "device_ms_per_batch": {"coding_phases_seen": int(t[0]), "clip_upload": round(t[2] / nph, 3), "load_pyramid": round(t[3] / nph, 3), "motion_search": round(t[4] / nph, 3),
                                        "table_uploads": round(t[5] / nph, 3), "coding_stream0": round(t[6] / nph, 3), "coding_stream1": round(t[7] / nph, 3),
                                        "fetch_gather_copy": round(t[8] / nph, 3), "coding_overlapped_by_load_or_search": round(t[11] / nph, 3)},
                "device_span_ms": round(t[1], 3),
                "device_idle_ms_per_batch": round(t[10] / nph, 3),
                "device_idle_note": "device time inside [first coding start, last coding end] with no load / motion-search / table-upload / coding phase in flight on any pipeline stream: the chip waiting for the host"}

    def prof_enable(self, kernels):
        """kernels: iterable of kernel names whose launches get HIP-event brackets (empty = off)"""
        names = self.kernel_names()
        mask = 0
        for k in kernels:
            mask |= 1 << names.index(k)
        _chk(self.L.dsvg_prof_enable(self.ctx, mask), "dsvg_prof_enable")
        _chk(self.L.dsvg_prof_reset(self.ctx), "dsvg_prof_reset")

    def prof_get(self, kernel):
        """(total ms, launches, algorithmic bytes) of one kernel since the last prof_enable"""
        kid = self.kernel_names().index(kernel)
        ms, n, by = _C.c_double(0), _C.c_long(0), _C.c_double(0)
        _chk(self.L.dsvg_prof_get(self.ctx, kid, _C.byref(ms), _C.byref(n), _C.byref(by)), "dsvg_prof_get")
        return ms.value, n.value, by.value

    def close(self):
        if self.h:
            for p in self._dev:
                self.L.dsvg_dev_free(self.ctx, p)
            self._dev = []
            self.L.dsvg_ctx_sync(self.ctx)
            for p in self._pin:
                self.L.dsvg_host_free(self.ctx, p)
            self._pin = []
            self.L.dsv1_batch_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ladder(Batch):
    """A quality ladder (dsv1_ladder_open): nsources sources, each coded at every rung of `rungs` (configs from make_encoder_cfg that
    differ only in their rate-control fields) from one upload and one analysis.  Input is [source][frame] (nsources x F frames);
    results -- encode() / collect() streams, sse(), ssim(), encoder(k), eos -- are per output stream k = source * nrungs + rung.
    set_fnum(k, n) renumbers every rung of k's source.  Otherwise the methods of Batch."""

    def __init__(self, rungs, nsources, frames_per_call, device=0):
        rungs = list(rungs)
        if not 1 <= len(rungs) <= MAX_RUNGS:
            raise ValueError("a ladder has 1 to %d rungs, got %d" % (MAX_RUNGS, len(rungs)))
        self.L = lib()
        self.h = _C.c_void_p(None)
        self.nrungs, self.nsources, self.F = len(rungs), nsources, frames_per_call
        self.nstreams = nsources * self.nrungs
        arr = (Encoder * self.nrungs)(*rungs)
        _chk(self.L.dsv1_ladder_open(_C.byref(self.h), arr, self.nrungs, device, nsources, frames_per_call), "dsv1_ladder_open")
        self._opened(rungs[0])

    def stage(self, yuv):
        """Batch.stage(), the clip checked for nsources x F frames (the upload reads that many)"""
        self._input(yuv)
        Batch.stage(self, yuv)

    def stream(self, source, rung):
        """output stream index k of (source, rung)"""
        return source * self.nrungs + rung


MAX_RUNGS = 16   # DSV1_MAX_RUNGS
MAX_GEOMS = 16   # DSV1_MAX_GEOMS
SCALE_TENT, SCALE_CUBIC = 0, 1   # DSV1_SCALE_TENT, DSV1_SCALE_CUBIC


def pix_frame_bytes(pf, w, h, fmt):
    """bytes from frame to frame of a clip of PixFormat pf (dsv1_pix_frame_bytes); ValueError for an invalid combination"""
    n = lib().dsv1_pix_frame_bytes(_C.byref(pf), w, h, fmt)
    if not n:
        raise ValueError("not a valid pixel format for %dx%d frames of subsampling 0x%x" % (w, h, fmt))
    return int(n)


def _host_clip(clip, fb, what="a clip", raw=False):
    """a host clip of fb-byte frames as (flat uint8 array, frames); raw: the clip's bytes as they lie, whatever its dtype"""
    a = (_np.ascontiguousarray(clip).view(_np.uint8) if raw else _np.ascontiguousarray(clip, dtype=_np.uint8)).reshape(-1)
    if a.size % fb or not a.size:
        raise ValueError("%s is a whole number of %d-byte frames, got %d bytes" % (what, fb, a.size))
    return a, a.size // fb


def _host_out(out, frames, dfb):
    """the exporters' result: `out` if it can hold frames x dfb bytes, or a zeroed array of that shape"""
    res = _np.zeros((frames, dfb), dtype=_np.uint8) if out is None else out
    if res.dtype != _np.uint8 or not res.flags.c_contiguous or res.size < frames * dfb:
        raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % (frames * dfb))
    return res


def convert_clip(clip, pf, w, h, fmt, device=0, n=None, out=None, src_fmt=None):
    """convert frames of PixFormat pf to packed planar 8-bit on the GPU (dsv1_convert_clip): clip numpy uint8 [frames][frame bytes]
    (host), or a device pointer with n frames and `out` a device pointer for the result.  Host input returns numpy uint8
    [frames][planar frame_bytes].  src_fmt: the subsampling of the clip where it is not fmt (dsv1_convert_clip_sub) -- 4:4:4 or 4:2:2,
    chroma halved to fmt in the same pass."""
    L = lib()
    if src_fmt is None:
        call, what, sub = L.dsv1_convert_clip, "dsv1_convert_clip", (fmt,)
    else:
        call, what, sub = L.dsv1_convert_clip_sub, "dsv1_convert_clip_sub", (src_fmt, fmt)
    sfb = pix_frame_bytes(pf, w, h, sub[0])
    dfb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is not None:
        _chk(call(device, clip, _C.byref(pf), w, h, *sub, n, out, 1), what)
        return out
    a, frames = _host_clip(clip, sfb, "a clip of this format", raw=True)
    res = _np.zeros((frames, dfb), dtype=_np.uint8)
    _chk(call(device, a.ctypes.data, _C.byref(pf), w, h, *sub, frames, res.ctypes.data, 0), what)
    return res


def deinterlace_clip(clip, w, h, fmt, di, prev=None, device=0, n=None, out=None):
    """deinterlace packed planar 8-bit frames of one stream on the GPU (dsv1_deinterlace_clip) as Deint di says: clip numpy uint8
    [frames][frame_bytes] and prev one frame or None (host), or device pointers with n frames and `out` a device pointer for the
    result.  Host input returns numpy uint8 [frames or 2 x frames][frame_bytes]."""
    L = lib()
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is not None:
        _chk(L.dsv1_deinterlace_clip(device, clip, w, h, fmt, n, prev, out, _C.byref(di), 1), "dsv1_deinterlace_clip")
        return out
    a, frames = _host_clip(clip, fb)
    nout = L.dsv1_deint_out_frames(_C.byref(di), frames)
    if nout < 0:
        raise ValueError("not a deinterlacer: mode %d, tff %d" % (di.mode, di.tff))
    p = None
    if prev is not None:
        p = _np.ascontiguousarray(prev, dtype=_np.uint8).reshape(-1)
        if p.size != fb:
            raise ValueError("prev is one frame of %d bytes, got %d" % (fb, p.size))
    res = _np.zeros((nout, fb), dtype=_np.uint8)
    _chk(L.dsv1_deinterlace_clip(device, a.ctypes.data, w, h, fmt, frames, p.ctypes.data if p is not None else None, res.ctypes.data,
                                 _C.byref(di), 0), "dsv1_deinterlace_clip")
    return res


def ivtc_out_frames(iv, n):
    """4n / 5, the pictures n telecined frames leave (dsv1_ivtc_out_frames); ValueError unless iv is valid and n a multiple of 5"""
    r = lib().dsv1_ivtc_out_frames(_C.byref(iv), n)
    if r < 0:
        raise ValueError("not an inverse telecine call: tff %d, nt %d, %d frames" % (iv.tff, iv.nt, n))
    return r


def ivtc_clip(clip, w, h, fmt, iv, state=None, device=0, n=None, out=None, state_out=None):
    """inverse telecine of packed planar 8-bit frames of one stream on the GPU (dsv1_ivtc_clip) as Ivtc iv says: clip numpy uint8
    [5k frames][frame_bytes] and state what the call before returned or None (host), which returns (pictures numpy uint8
    [4k][frame_bytes], match uint8 [5k], drop uint8 [k], state uint8 [frame_bytes + w * h]); or device pointers with n frames, `out` a
    device pointer for the result and state / state_out device pointers or None, which returns (out, match, drop)."""
    L = lib()
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    sb = fb + w * h
    frames = n if n is not None else _host_clip(clip, fb)[1]
    nout = ivtc_out_frames(iv, frames)
    match = _np.zeros(frames, dtype=_np.uint8)
    drop = _np.zeros(frames // 5, dtype=_np.uint8)
    if n is not None:
        _chk(L.dsv1_ivtc_clip(device, clip, w, h, fmt, n, state, state_out, out, _C.byref(iv), match.ctypes.data, drop.ctypes.data, 1), "dsv1_ivtc_clip")
        return out, match, drop
    a, frames = _host_clip(clip, fb)
    p = None
    if state is not None:
        p = _np.ascontiguousarray(state, dtype=_np.uint8).reshape(-1)
        if p.size != sb:
            raise ValueError("a state is %d bytes, got %d" % (sb, p.size))
    res = _np.zeros((nout, fb), dtype=_np.uint8)
    new = _np.zeros(sb, dtype=_np.uint8)
    _chk(L.dsv1_ivtc_clip(device, a.ctypes.data, w, h, fmt, frames, p.ctypes.data if p is not None else None, new.ctypes.data, res.ctypes.data,
                          _C.byref(iv), match.ctypes.data, drop.ctypes.data, 0), "dsv1_ivtc_clip")
    return res, match, drop, new


def field_metrics_clip(clip, w, h, fmt, prev=None, nt=0, device=0, n=None):
    """the four comb sums mc0 mc1 mp0 mp1 of every frame's luma, on the GPU (dsv1_field_metrics_clip): clip numpy uint8
    [frames][frame_bytes] and prev one frame or None (host), or device pointers with n frames.  Returns numpy uint32 [frames][4]."""
    L = lib()
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is None:
        a, frames = _host_clip(clip, fb)
        src, dev = a.ctypes.data, 0
        if prev is not None:
            pa = _np.ascontiguousarray(prev, dtype=_np.uint8).reshape(-1)
            if pa.size != fb:
                raise ValueError("prev is one frame of %d bytes, got %d" % (fb, pa.size))
            prev = pa.ctypes.data
    else:
        src, frames, dev = clip, n, 1
    met = _np.zeros((max(frames, 0), 4), dtype=_np.uint32)
    _chk(L.dsv1_field_metrics_clip(device, src, w, h, fmt, frames, prev, nt, met.ctypes.data, dev), "dsv1_field_metrics_clip")
    return met


def field_order_from_metrics(metrics, first_has_prev=False):
    """the field order a clip's metrics vote for (dsv1_field_order_from_metrics): 1 top field first, 0 bottom field first, -1
    undetermined (static or progressive material, or texture too fine for the motion).  Host only."""
    m = _np.ascontiguousarray(metrics, dtype=_np.uint32).reshape(-1, 4)
    r = lib().dsv1_field_order_from_metrics(m.ctypes.data, m.shape[0], 1 if first_has_prev else 0)
    if r < -1:
        raise ValueError("dsv1_field_order_from_metrics refused %d frames (rc=%d)" % (m.shape[0], r))
    return r


def detect_field_order_clip(clip, w, h, fmt, nt=0, device=0, n=None):
    """field metrics on the GPU and the vote in one call (dsv1_detect_field_order_clip): 1 / 0 / -1"""
    L = lib()
    if n is None:
        a, frames = _host_clip(clip, w * h + 2 * _chroma_size(w, h, fmt))
        src, dev = a.ctypes.data, 0
    else:
        src, frames, dev = clip, n, 1
    r = L.dsv1_detect_field_order_clip(device, src, w, h, fmt, frames, nt, dev)
    if r < -1:
        _chk(r, "dsv1_detect_field_order_clip")
    return r


def denoise_clip(clip, w, h, fmt, dn, state=None, device=0, n=None, out=None, state_out=None):
    """temporal noise reduction of packed planar 8-bit pictures of one stream on the GPU (dsv1_denoise_clip) as Denoise dn says: clip
    numpy uint8 [pictures][frame_bytes] and state what the call before returned or None (host), which returns (numpy uint8
    [pictures][frame_bytes], state numpy uint8 [3 x frame_bytes]); or device pointers with n pictures, `out` a device pointer for the
    result and state / state_out device pointers or None, which returns out."""
    L = lib()
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is not None:
        _chk(L.dsv1_denoise_clip(device, clip, w, h, fmt, n, state, state_out, out, _C.byref(dn), 1), "dsv1_denoise_clip")
        return out
    a, frames = _host_clip(clip, fb)
    p = None
    if state is not None:
        p = _np.ascontiguousarray(state, dtype=_np.uint8).reshape(-1)
        if p.size != 3 * fb:
            raise ValueError("a state is %d bytes, got %d" % (3 * fb, p.size))
    res = _np.zeros((frames, fb), dtype=_np.uint8)
    new = _np.zeros(3 * fb, dtype=_np.uint8)
    _chk(L.dsv1_denoise_clip(device, a.ctypes.data, w, h, fmt, frames, p.ctypes.data if p is not None else None, new.ctypes.data,
                             res.ctypes.data, _C.byref(dn), 0), "dsv1_denoise_clip")
    return res, new


def reframe_clip(clip, rf, fmt, device=0, n=None, out=None):
    """reframe packed planar 8-bit frames on the GPU (dsv1_reframe_clip) as Reframe rf says: clip numpy uint8 [frames][frame bytes of
    rf.in_w x rf.in_h] (host), which returns numpy uint8 [frames][frame bytes of rf.out_w x rf.out_h]; or a device pointer with n
    frames and `out` a device pointer for the result."""
    L = lib()
    if n is not None:
        _chk(L.dsv1_reframe_clip(device, clip, n, out, _C.byref(rf), fmt, 1), "dsv1_reframe_clip")
        return out
    if not L.dsv1_reframe_valid(_C.byref(rf), fmt):
        raise ValueError("not a valid reframe at subsampling 0x%x" % fmt)
    a, frames = _host_clip(clip, rf.in_w * rf.in_h + 2 * _chroma_size(rf.in_w, rf.in_h, fmt))
    res = _host_out(out, frames, rf.out_w * rf.out_h + 2 * _chroma_size(rf.out_w, rf.out_h, fmt))
    _chk(L.dsv1_reframe_clip(device, a.ctypes.data, frames, res.ctypes.data, _C.byref(rf), fmt, 0), "dsv1_reframe_clip")
    return res


def orient_dims(orient, w, h):
    """(width, height) of w x h frames oriented by code `orient` (dsv1_orient_dims)"""
    ow, oh = _C.c_int(0), _C.c_int(0)
    if lib().dsv1_orient_dims(orient, w, h, _C.byref(ow), _C.byref(oh)):
        raise ValueError("orient_dims: code %d / %dx%d refused" % (orient, w, h))
    return ow.value, oh.value


def _orient_code(rc, what):
    if rc < 0:
        raise ValueError("%s refused (rc=%d)" % (what, rc))
    return rc


def orient_compose(a, b):
    """the one code equal to applying a and then b (dsv1_orient_compose)"""
    return _orient_code(lib().dsv1_orient_compose(a, b), "orient_compose(%d, %d)" % (a, b))


def orient_inverse(a):
    """the code that undoes a (dsv1_orient_inverse)"""
    return _orient_code(lib().dsv1_orient_inverse(a), "orient_inverse(%d)" % a)


def orient_from_exif(tag):
    """EXIF orientation tag 1 .. 8 -> code (dsv1_orient_from_exif)"""
    return _orient_code(lib().dsv1_orient_from_exif(tag), "orient_from_exif(%d)" % tag)


def orient_from_matrix(m):
    """an MP4 / QuickTime track display matrix (9 int32, 16.16 fixed point) -> code (dsv1_orient_from_matrix); scale, shear and other
    angles raise ValueError"""
    m = [int(x) for x in m]
    if len(m) != 9:
        raise ValueError("a display matrix has 9 entries")
    return _orient_code(lib().dsv1_orient_from_matrix((_C.c_int32 * 9)(*m)), "orient_from_matrix")


def orient_clip(clip, w, h, fmt, orient, device=0, n=None, out=None):
    """orient packed planar 8-bit frames of w x h on the GPU (dsv1_orient_clip) by code `orient`: clip numpy uint8 [frames][frame
    bytes] (host), which returns numpy uint8 [frames][frame bytes] of orient_dims(orient, w, h); or a device pointer with n frames and
    `out` a device pointer for the result.  Code 0 copies."""
    L = lib()
    if n is not None:
        _chk(L.dsv1_orient_clip(device, clip, w, h, fmt, n, out, orient, 1), "dsv1_orient_clip")
        return out
    if not L.dsv1_orient_valid(orient, fmt):
        raise ValueError("%d is not an orientation at subsampling 0x%x" % (orient, fmt))
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    a, frames = _host_clip(clip, fb)
    res = _host_out(out, frames, fb)
    _chk(L.dsv1_orient_clip(device, a.ctypes.data, w, h, fmt, frames, res.ctypes.data, orient, 0), "dsv1_orient_clip")
    return res


def levels_clip(clip, w, h, fmt, lv, device=0, n=None, out=None):
    """pass packed planar 8-bit frames of w x h through Levels lv on the GPU (dsv1_levels_clip): clip numpy uint8 [frames][frame bytes]
    (host), which returns numpy uint8 [frames][frame bytes]; or a device pointer with n frames and `out` a device pointer for the
    result.  `out` may be the clip itself."""
    L = lib()
    if n is not None:
        _chk(L.dsv1_levels_clip(device, clip, w, h, fmt, n, out, _C.byref(lv), 1), "dsv1_levels_clip")
        return out
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    a, frames = _host_clip(clip, fb)
    res = _host_out(out, frames, fb)
    _chk(L.dsv1_levels_clip(device, a.ctypes.data, w, h, fmt, frames, res.ctypes.data, _C.byref(lv), 0), "dsv1_levels_clip")
    return res


def histogram_clip(clip, w, h, fmt, device=0, n=None):
    """the histogram of every plane of every frame of a clip, on the GPU (dsv1_histogram_clip): clip numpy uint8 [frames][frame_bytes]
    (host), or a device pointer with n frames.  Returns numpy uint32 [frames][3][256]."""
    L = lib()
    if n is None:
        a, frames = _host_clip(clip, w * h + 2 * _chroma_size(w, h, fmt))
        src, dev = a.ctypes.data, 0
    else:
        src, frames, dev = clip, n, 1
    hist = _np.zeros((max(frames, 0), 3, 256), dtype=_np.uint32)
    _chk(L.dsv1_histogram_clip(device, src, w, h, fmt, frames, hist.ctypes.data, dev), "dsv1_histogram_clip")
    return hist


def _hist(hist):
    g = _np.ascontiguousarray(hist, dtype=_np.uint32)
    if g.ndim < 2 or g.shape[-2:] != (3, 256) or not g.size:
        raise ValueError("a histogram is uint32 [frames][3][256]")
    return g, g.size // 768


def range_from_histogram(hist, ppm=1000):
    """True where more than ppm millionths of the samples lie outside the limited range (dsv1_range_from_histogram): full-range.
    Host only."""
    g, n = _hist(hist)
    full = _C.c_int(0)
    if lib().dsv1_range_from_histogram(g.ctypes.data, n, ppm, _C.byref(full)):
        raise ValueError("dsv1_range_from_histogram: ppm %d refused" % ppm)
    return bool(full.value)


def points_from_histogram(hist, low_ppm=1000, high_ppm=1000):
    """(black, white) of the luma: at most low_ppm millionths of the samples lie below black, high_ppm above white
    (dsv1_points_from_histogram), or None where black >= white.  Host only."""
    g, n = _hist(hist)
    b, w = _C.c_int(0), _C.c_int(0)
    rc = lib().dsv1_points_from_histogram(g.ctypes.data, n, low_ppm, high_ppm, _C.byref(b), _C.byref(w))
    if rc < 0:
        raise ValueError("dsv1_points_from_histogram: ppm %d / %d refused" % (low_ppm, high_ppm))
    return (b.value, w.value) if rc else None


def detect_range_clip(clip, w, h, fmt, ppm=1000, device=0, n=None):
    """the histogram on the GPU and the range rule in one call (dsv1_detect_range_clip): True for a full-range clip"""
    L = lib()
    if n is None:
        a, frames = _host_clip(clip, w * h + 2 * _chroma_size(w, h, fmt))
        src, dev = a.ctypes.data, 0
    else:
        src, frames, dev = clip, n, 1
    full = _C.c_int(0)
    _chk(L.dsv1_detect_range_clip(device, src, w, h, fmt, frames, ppm, _C.byref(full), dev), "dsv1_detect_range_clip")
    return bool(full.value)


def overlay_bytes(w, h, fmt):
    """the bytes of an overlay bitmap's four planes (dsv1_overlay_bytes)"""
    return int(lib().dsv1_overlay_bytes(w, h, fmt))


def overlay_valid(ov, W, H, fmt, nsources=1):
    """whether Overlay ov is valid on a canvas of W x H in format fmt in a session of nsources sources (dsv1_overlay_valid).  Host only."""
    return bool(lib().dsv1_overlay_valid(_C.byref(ov), W, H, fmt, nsources))


def overlay_opacity_at(ov, t):
    """the opacity, 0 .. 256, Overlay ov has on picture t (dsv1_overlay_opacity_at).  Host only."""
    return int(lib().dsv1_overlay_opacity_at(_C.byref(ov), t))


def overlay_plan(overlays, nsources, frames, counters, W, H, fmt):
    """the plan of one call (dsv1_overlay_plan): ([(overlay, source, frame, op, layer), ...] in the order source, frame, overlay,
    layers).  counters: every source's picture counter at the call's first frame.  Host only."""
    arr, n = _overlay_array(overlays)
    cnt = (_C.c_int64 * nsources)(*[int(c) for c in counters])
    L = lib()
    need = L.dsv1_overlay_plan(arr, n, nsources, frames, cnt, W, H, fmt, None, 0, None)
    if need < 0:
        raise ValueError("dsv1_overlay_plan refused the list (rc=%d)" % need)
    items = (OverlayItem * max(need, 1))()
    layers = _C.c_int(0)
    got = L.dsv1_overlay_plan(arr, n, nsources, frames, cnt, W, H, fmt, items, need, _C.byref(layers))
    assert got == need
    return [(it.overlay, it.source, it.frame, it.op, it.layer) for it in items[:need]], layers.value


class SubmitSrc(_C.Structure):
    """dsv1_submit_src: a source's decision state"""
    _fields_ = [("next_fnum", _C.c_uint32), ("prev_gop", _C.c_uint32), ("gop", _C.c_int), ("force_metadata", _C.c_int),
                ("do_scd", _C.c_int), ("prev_avg_luma", _C.c_int), ("scene_change_delta", _C.c_int)]


class SubmitPic(_C.Structure):
    """dsv1_submit_pic: a picture's decisions"""
    _fields_ = [("fnum", _C.c_uint32), ("gop_start", _C.c_int), ("is_ref", _C.c_int), ("has_ref", _C.c_int), ("forced_intra", _C.c_int),
                ("isP", _C.c_int), ("n_intra", _C.c_int), ("reach", _C.c_short * 4), ("cur_slot", _C.c_int), ("ref_slot", _C.c_int),
                ("out_slot", _C.c_int)]


class SubmitStream(_C.Structure):
    """dsv1_submit_stream: an output stream's state"""
    _fields_ = [("rpar", _C.c_ubyte), ("has_recon", _C.c_ubyte), ("border_skipped", _C.c_ubyte), ("recon_dropped", _C.c_ubyte),
                ("next_gop", _C.c_ubyte)]


class SubmitJob(_C.Structure):
    """dsv1_submit_job: one device job of a submit's plan"""
    _fields_ = [("pic", _C.c_int), ("ref_recon_slot", _C.c_int), ("recon_slot", _C.c_int), ("out_slot", _C.c_int),
                ("border_hint", _C.c_int), ("remedy", _C.c_int)]


class SubmitCall(_C.Structure):
    """dsv1_submit_call: nsteps frame steps of njobs jobs each, from job `first` on"""
    _fields_ = [("nsteps", _C.c_int), ("njobs", _C.c_int), ("first", _C.c_int)]


class SubmitQuery(_C.Structure):
    """dsv1_submit_query: the geometry and mode of one submit, and how much of each table its plan wrote"""
    _fields_ = [("S", _C.c_int), ("R", _C.c_int), ("F", _C.c_int), ("nf", _C.c_int), ("chains", _C.c_int), ("gcount", _C.c_uint),
                ("par", _C.c_int), ("npix_small", _C.c_int), ("nblk", _C.c_int), ("intra_pct_thresh", _C.c_int), ("abr", _C.c_int),
                ("serial", _C.c_int), ("keep_all", _C.c_int), ("nf_prev", _C.c_int), ("carry", _C.c_int * 2), ("npairs", _C.c_int),
                ("next", _C.c_int), ("nremedy", _C.c_int), ("njobs", _C.c_int), ("ncalls", _C.c_int), ("dropped", _C.c_int)]


class SubmitTables(_C.Structure):
    """dsv1_submit_tables: the tables a plan writes"""
    _fields_ = [("pics", _C.POINTER(SubmitPic)), ("pair_cur", _C.POINTER(_C.c_int)), ("pair_ref", _C.POINTER(_C.c_int)),
                ("pair_pic", _C.POINTER(_C.c_int)), ("ext", _C.POINTER(_C.c_int)), ("remedy_streams", _C.POINTER(_C.c_int)),
                ("remedy", _C.POINTER(SubmitJob)), ("jobs", _C.POINTER(SubmitJob)), ("calls", _C.POINTER(SubmitCall)),
                ("scratch", _C.POINTER(_C.c_int))]


def _fields(x):
    return {n: (list(getattr(x, n)) if hasattr(getattr(x, n), "__len__") else int(getattr(x, n))) for n, _ in x._fields_}


def submit_plan(q, src, st, luma, n_intra, prev=None):
    """the plan of one submit (dsv1_submit_plan), no device.  q: SubmitQuery; src: list of SubmitSrc, one per source; st: list of
    SubmitStream, one per output stream -- all three are updated as the submit would leave them.  luma: raw luma sums by source slot
    ((2F + 1) * S of them); n_intra[stream * F + t]: the intra blocks of a motion-search candidate; prev: the SubmitPic array the call
    before returned as ["_pics"].  Returns a dict of lists of dicts: pics, pairs (cur, ref, pic), ext, remedy_streams, remedy, jobs,
    calls, and dropped.  Raises ValueError where the submit is refused."""
    S, R, F = q.S, q.R, q.F
    N = S * R
    a_src = (SubmitSrc * S)(*src)
    a_st = (SubmitStream * N)(*st)
    a_luma = (_C.c_uint * ((2 * F + 1) * S))(*[int(v) for v in luma])
    a_ni = (_C.c_int * (N * F))(*[int(v) for v in n_intra])
    pics = (SubmitPic * (N * F))()
    pc, pr, pp = (_C.c_int * (S * F))(), (_C.c_int * (S * F))(), (_C.c_int * (S * F))()
    ext = (_C.c_int * N)()
    rem, jobs, calls = (SubmitJob * N)(), (SubmitJob * (N * F))(), (SubmitCall * F)()
    scratch = (_C.c_int * (4 * (F + 1)))()
    rems = (_C.c_int * N)()
    P = _C.POINTER
    tb = SubmitTables(pics, pc, pr, pp, ext, rems, rem, jobs, calls, scratch)
    L = lib()
    L.dsv1_submit_plan.restype = _C.c_int
    L.dsv1_submit_plan.argtypes = [P(SubmitQuery), P(SubmitSrc), P(SubmitStream), P(_C.c_uint), P(_C.c_int), P(SubmitPic), P(SubmitTables)]
    rc = L.dsv1_submit_plan(_C.byref(q), a_src, a_st, a_luma, a_ni, prev, _C.byref(tb))
    if rc:
        raise ValueError("dsv1_submit_plan refused the call (rc=%d)" % rc)
    for i in range(S):
        src[i] = a_src[i]
    for i in range(N):
        st[i] = a_st[i]
    return {"_pics": pics, "pics": [_fields(p) for p in pics],
            "pairs": [(pc[i], pr[i], pp[i]) for i in range(q.npairs)], "ext": list(ext[:q.next]),
            "remedy_streams": list(rems[:q.nremedy]), "remedy": [_fields(j) for j in rem[:q.nremedy]],
            "jobs": [_fields(j) for j in jobs[:q.njobs]], "calls": [_fields(c) for c in calls[:q.ncalls]], "dropped": q.dropped}


SC_NONE, SC_CONVERT, SC_LEVELS, SC_DEINTERLACE, SC_IVTC, SC_DENOISE, SC_ORIENT, SC_REFRAME, SC_OVERLAY = range(9)
SC_SLOTS, SC_MAX_STEPS = 7, 8
SC_OP_SET, SC_OP_RESET, SC_OP_SEEK = range(3)
SC_CALLER, SC_UPLOAD = -1, -2


class SrcChainState(_C.Structure):
    """dsv1_srcchain_state: a session's source chain as plain data"""
    _fields_ = [("nsrc", _C.c_int), ("F", _C.c_int), ("subsamp", _C.c_int), ("keep_lane", _C.c_int), ("ow", _C.c_int), ("oh", _C.c_int),
                ("kind", _C.c_int * SC_SLOTS), ("conv_rgb", _C.c_int), ("conv_fb", _C.c_size_t), ("deint_mode", _C.c_int),
                ("orient", _C.c_int), ("in_w", _C.c_int), ("in_h", _C.c_int), ("ov_clip", _C.c_int * 2)]


class SrcChainReq(_C.Structure):
    """dsv1_srcchain_req: one setter, reset or seek call, its numbers resolved"""
    _fields_ = [("op", _C.c_int), ("kind", _C.c_int), ("set", _C.c_int), ("valid", _C.c_int), ("identity", _C.c_int), ("busy", _C.c_int),
                ("mode", _C.c_int), ("w", _C.c_int), ("h", _C.c_int), ("out_w", _C.c_int), ("out_h", _C.c_int), ("source", _C.c_int),
                ("frame_bytes", _C.c_size_t)]


class SrcChainGeom(_C.Structure):
    """dsv1_srcchain_geom: the three geometries of a chain state and what a call brings"""
    _fields_ = [("w", _C.c_int), ("h", _C.c_int), ("mw", _C.c_int), ("mh", _C.c_int), ("ow", _C.c_int), ("oh", _C.c_int),
                ("conv_frames", _C.c_int), ("frames_in", _C.c_int), ("lane", _C.c_int), ("fb", _C.c_size_t), ("mfb", _C.c_size_t),
                ("ofb", _C.c_size_t), ("frame_in_bytes", _C.c_size_t), ("bytes_in", _C.c_size_t)]


class SrcChainSetPlan(_C.Structure):
    """dsv1_srcchain_set_plan: the answer to a request"""
    _fields_ = [("rc", _C.c_int), ("text", _C.c_int), ("noop", _C.c_int), ("next", SrcChainState), ("g", SrcChainGeom),
                ("alloc", _C.c_size_t * SC_SLOTS), ("free_", _C.c_int * SC_SLOTS), ("reset", _C.c_int * SC_SLOTS)]


class SrcChainStep(_C.Structure):
    """dsv1_srcchain_step: one enqueued step of a call"""
    _fields_ = [("kind", _C.c_int), ("pos", _C.c_int), ("nframes", _C.c_int), ("src", _C.c_int), ("dst", _C.c_int),
                ("bytes", _C.c_size_t), ("alloc", _C.c_size_t)]


class SrcChainCallPlan(_C.Structure):
    """dsv1_srcchain_call_plan: one call's clip through the chain"""
    _fields_ = [("rc", _C.c_int), ("bypass", _C.c_int), ("nsteps", _C.c_int), ("out", _C.c_int), ("advance", _C.c_int),
                ("upload", _C.c_size_t), ("step", SrcChainStep * SC_MAX_STEPS)]


class SrcChainRefused(ValueError):
    """the source chain refuses the request or the call: rc and text are what the session would return and log"""
    def __init__(self, rc, row, text):
        super().__init__("the source chain refuses (rc=%d): %s" % (rc, text))
        self.rc, self.row, self.text = rc, row, text


_SC = {}


def _sc():
    """the three source-chain plan entry points, bound once, and the table's rows"""
    if not _SC:
        L, P = lib(), _C.POINTER
        L.dsv1_srcchain_plan_text.restype, L.dsv1_srcchain_plan_text.argtypes = _C.c_char_p, [_C.c_int]
        L.dsv1_srcchain_plan_set.restype, L.dsv1_srcchain_plan_set.argtypes = _C.c_int, [P(SrcChainState), P(SrcChainReq), P(SrcChainSetPlan)]
        L.dsv1_srcchain_plan_call.restype = _C.c_int
        L.dsv1_srcchain_plan_call.argtypes = [P(SrcChainState), _C.c_int, _C.c_int, _C.c_int, P(SrcChainCallPlan)]
        texts = []
        while L.dsv1_srcchain_plan_text(len(texts)) is not None:
            texts.append(L.dsv1_srcchain_plan_text(len(texts)).decode())
        _SC.update(set=L.dsv1_srcchain_plan_set, call=L.dsv1_srcchain_plan_call, texts=texts)
    return _SC


def srcchain_plan_texts():
    """the rows of the chain's refusal table (dsv1_srcchain_plan_text); row 0 (no refusal) is empty"""
    return list(_sc()["texts"])


def srcchain_plan_set(state, req):
    """the plan of one setter, reset or seek call (dsv1_srcchain_plan_set), no device: a SrcChainSetPlan; SrcChainRefused where the
    session refuses"""
    out = SrcChainSetPlan()
    out.text = -1
    rc = _sc()["set"](_C.byref(state), _C.byref(req), _C.byref(out))
    if rc and out.text < 0:
        raise ValueError("not a request of the source chain: op %d of kind %d" % (req.op, req.kind))
    if rc:
        raise SrcChainRefused(rc, out.text, _SC["texts"][out.text])
    return out


def srcchain_plan_call(state, form, active, par=0):
    """the plan of one call (dsv1_srcchain_plan_call), no device.  form: 0 host, 1 plain device clip, 2 held; active: the overlays
    blend something in it.  A SrcChainCallPlan; SrcChainRefused for a chain without a lane"""
    out = SrcChainCallPlan()
    rc = _sc()["call"](_C.byref(state), form, 1 if active else 0, par, _C.byref(out))
    if rc:
        raise SrcChainRefused(rc, 0, "no lane: nothing is set")
    return out


def overlay_from_rgba(rgba, w, h, order, matrix, full_range, fmt, pitch=0):
    """an overlay bitmap's planes (numpy uint8: Y, U, V, A) from an RGB(A) image of w x h in memory order `order` (RGB_*), converted
    with `matrix` (MATRIX_*) at full or limited range to format fmt (dsv1_overlay_from_rgba).  Host only."""
    a = _np.ascontiguousarray(rgba, dtype=_np.uint8).reshape(-1)
    out = _np.zeros(overlay_bytes(w, h, fmt), dtype=_np.uint8)
    if not out.size or lib().dsv1_overlay_from_rgba(a.ctypes.data, pitch, w, h, order, matrix, full_range, fmt, out.ctypes.data):
        raise ValueError("dsv1_overlay_from_rgba refused %dx%d order %d matrix %d range %d format 0x%x" % (w, h, order, matrix, full_range, fmt))
    return out


def overlay_clip(clip, w, h, fmt, overlays, t_first=0, device=0, n=None):
    """blend the Overlay objects of a list onto packed planar 8-bit frames of w x h on the GPU (dsv1_overlay_clip); frame i is picture
    t_first + i of source 0.  clip numpy uint8 [frames][frame bytes] (host): returns the composited copy; or a device pointer with n
    frames: blended in place."""
    L = lib()
    arr, cnt = _overlay_array(overlays)
    if n is not None:
        _chk(L.dsv1_overlay_clip(device, clip, w, h, fmt, n, arr, cnt, t_first, 1), "dsv1_overlay_clip")
        return clip
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    a, frames = _host_clip(clip, fb)
    res = a.reshape(frames, fb).copy()
    _chk(L.dsv1_overlay_clip(device, res.ctypes.data, w, h, fmt, frames, arr, cnt, t_first, 0), "dsv1_overlay_clip")
    return res


def line_sums_clip(clip, w, h, fmt, device=0, n=None):
    """the sums of every luma row and column of a clip, on the GPU (dsv1_line_sums_clip): clip numpy uint8 [frames][frame_bytes]
    (host), or a device pointer with n frames.  Returns (row_sum numpy uint32 [frames][h], col_sum numpy uint32 [frames][w])."""
    L = lib()
    if n is None:
        a, frames = _host_clip(clip, w * h + 2 * _chroma_size(w, h, fmt))
        src, dev = a.ctypes.data, 0
    else:
        src, frames, dev = clip, n, 1
    rows = _np.zeros((max(frames, 0), h), dtype=_np.uint32)
    cols = _np.zeros((max(frames, 0), w), dtype=_np.uint32)
    _chk(L.dsv1_line_sums_clip(device, src, w, h, fmt, frames, rows.ctypes.data, cols.ctypes.data, dev), "dsv1_line_sums_clip")
    return rows, cols


def bars_from_sums(row_sum, col_sum, thresh=24, align=2):
    """the content rectangle (x, y, w, h) of a clip from its line sums (dsv1_bars_from_sums; ffmpeg cropdetect's rule: a line is
    content if its mean exceeds thresh in any frame; rounded inward to `align`), or None when nothing is content.  Host only."""
    r = _np.ascontiguousarray(row_sum, dtype=_np.uint32)
    c = _np.ascontiguousarray(col_sum, dtype=_np.uint32)
    r, c = r.reshape(-1, r.shape[-1]), c.reshape(-1, c.shape[-1])
    if r.shape[0] != c.shape[0]:
        raise ValueError("row sums of %d frames, column sums of %d" % (r.shape[0], c.shape[0]))
    rect = (_C.c_int * 4)()
    rc = lib().dsv1_bars_from_sums(r.ctypes.data, c.ctypes.data, c.shape[1], r.shape[1], r.shape[0], thresh, align, rect)
    if rc < 0:
        raise ValueError("dsv1_bars_from_sums: thresh %d / align %d refused (rc=%d)" % (thresh, align, rc))
    return tuple(rect) if rc else None


def detect_bars_clip(clip, w, h, fmt, thresh=24, align=2, device=0, n=None):
    """line sums on the GPU and the bars rule in one call (dsv1_detect_bars_clip): the content rectangle (x, y, w, h) or None"""
    L = lib()
    if n is None:
        a, frames = _host_clip(clip, w * h + 2 * _chroma_size(w, h, fmt))
        src, dev = a.ctypes.data, 0
    else:
        src, frames, dev = clip, n, 1
    rect = (_C.c_int * 4)()
    rc = L.dsv1_detect_bars_clip(device, src, w, h, fmt, frames, thresh, align, rect, dev)
    if rc < 0:
        _chk(rc, "dsv1_detect_bars_clip")
    return tuple(rect) if rc else None


def export_clip(clip, w, h, fmt, pf, out_subsamp=None, device=0, n=None, out=None, upsample=None):
    """packed planar 8-bit frames (w x h at subsampling fmt) to frames of PixFormat pf at subsampling out_subsamp (None: fmt) on the
    GPU (dsv1_export_clip), chroma halved on the way where out_subsamp asks for it: clip numpy uint8 [frames][frame_bytes] (host), or
    a device pointer with n frames and `out` a device pointer for the result.  Host input returns numpy uint8 [frames][frame bytes
    of pf]; `out` (a numpy uint8 array of that size) is written in place -- what the format pads stays as it was.  upsample
    (CHROMA_REPLICATE / CHROMA_LINEAR; dsv1_export_clip_up): out_subsamp may also be a finer one than fmt, chroma doubled that way."""
    L = lib()
    osub = fmt if out_subsamp is None else out_subsamp
    sfb = w * h + 2 * _chroma_size(w, h, fmt)
    if upsample is None:
        call, what, tail = L.dsv1_export_clip, "dsv1_export_clip", (osub,)
    else:
        call, what, tail = L.dsv1_export_clip_up, "dsv1_export_clip_up", (osub, upsample)
    if n is not None:
        _chk(call(device, clip, w, h, fmt, n, out, _C.byref(pf), *tail, 1), what)
        return out
    a, frames = _host_clip(clip, sfb, "a planar clip", raw=True)
    res = _host_out(out, frames, pix_frame_bytes(pf, w, h, osub))
    _chk(call(device, a.ctypes.data, w, h, fmt, frames, res.ctypes.data, _C.byref(pf), *tail, 0), what)
    return res


def packet_blockinfo(packet, w, h, n=None):
    """the side information of one picture packet of a w x h stream (dsv1_packet_blockinfo; host only): (blk_w, blk_h, has_ref, table),
    table a numpy array of BLOCKINFO_DTYPE, one entry per block in raster order (mode 0 inter / 1 intra; without a reference only
    `stable` is filled).  n: the room offered (None: enough for 16 x 16 blocks).  ValueError for anything but a well-formed picture
    packet, or too small an n."""
    data = _np.frombuffer(bytes(packet), dtype=_np.uint8)
    room = ((w + 15) // 16) * ((h + 15) // 16) if n is None else n
    tab = _np.zeros(max(room, 1), dtype=BLOCKINFO_DTYPE)
    bw, bh, ref = _C.c_int(0), _C.c_int(0), _C.c_int(0)
    rc = lib().dsv1_packet_blockinfo(data.ctypes.data, data.size, w, h, _C.byref(bw), _C.byref(bh), _C.byref(ref), tab.ctypes.data, room)
    if rc != 0:
        raise ValueError("not a picture packet of a %dx%d stream that %d entries can describe (rc=%d)" % (w, h, room, rc))
    nblk = ((w + bw.value - 1) // bw.value) * ((h + bh.value - 1) // bh.value)
    return bw.value, bh.value, ref.value, tab[:nblk]


def draw_info_clip(clip, w, h, fmt, blk_w, blk_h, info, mode, device=0, n=None):
    """the decoders' debug overlay (dsv1_draw_info_clip) on packed planar 8-bit frames: clip numpy uint8 [frames][frame_bytes] (host;
    returns the drawn copy), or a device pointer with n frames, drawn in place.  info: BLOCKINFO_DTYPE entries, ceil(w / blk_w) *
    ceil(h / blk_h) per frame.  ValueError for arguments the library refuses."""
    L = lib()
    fb = w * h + 2 * _chroma_size(w, h, fmt)
    tab = _np.ascontiguousarray(info, dtype=BLOCKINFO_DTYPE).reshape(-1)
    if n is not None:
        frames, ptr, res = n, clip, clip
    else:
        a, frames = _host_clip(clip, fb)
        res = a.copy().reshape(frames, fb)
        ptr = res.ctypes.data
    nblk = ((w + max(blk_w, 1) - 1) // max(blk_w, 1)) * ((h + max(blk_h, 1) - 1) // max(blk_h, 1))
    if tab.size < nblk * frames:
        raise ValueError("info holds %d entries, %d frames of %d blocks need %d" % (tab.size, frames, nblk, nblk * frames))
    rc = L.dsv1_draw_info_clip(device, ptr, w, h, fmt, frames, blk_w, blk_h, tab.ctypes.data, mode, 0 if n is None else 1)
    if rc == -2:
        raise ValueError("dsv1_draw_info_clip refuses these arguments (block %dx%d, mode %d, subsampling 0x%x)" % (blk_w, blk_h, mode, fmt))
    _chk(rc, "dsv1_draw_info_clip")
    return res


def rgb_frame_bytes(rf, w, h):
    """bytes from frame to frame of an RGB clip of RgbFormat rf (dsv1_rgb_frame_bytes); ValueError for an invalid format"""
    n = lib().dsv1_rgb_frame_bytes(_C.byref(rf), w, h)
    if not n:
        raise ValueError("not a valid RGB format for %dx%d frames" % (w, h))
    return int(n)


def rgb_tables(matrix, full_range):
    """(forward Q16 rows Y, Cb, Cr over R, G, B as int32 [3][3]; inverse Q14 IY, RV, GU, GV, BU as int32 [5]) the library holds
    (dsv1_rgb_tables; host only); ValueError for an unknown matrix or range"""
    fwd, inv = (_C.c_int32 * 9)(), (_C.c_int32 * 5)()
    if lib().dsv1_rgb_tables(matrix, full_range, fwd, inv) != 0:
        raise ValueError("no such matrix / range: %r, %r" % (matrix, full_range))
    return _np.array(fwd[:], dtype=_np.int32).reshape(3, 3), _np.array(inv[:], dtype=_np.int32)


def rgb_import_clip(clip, rf, w, h, fmt, device=0, n=None, out=None):
    """RGB frames of RgbFormat rf to packed planar 8-bit Y, Cb, Cr at subsampling fmt on the GPU (dsv1_rgb_import_clip): clip numpy uint8
    (host; a whole number of frames, the last one may end with its planes), or a device pointer with n frames and `out` a device
    pointer for the result.  Host input returns numpy uint8 [frames][planar frame_bytes]."""
    L = lib()
    sfb = rgb_frame_bytes(rf, w, h)
    dfb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is not None:
        _chk(L.dsv1_rgb_import_clip(device, clip, _C.byref(rf), w, h, fmt, n, out, 1), "dsv1_rgb_import_clip")
        return out
    a, frames = _host_clip(clip, sfb, "a clip of this format", raw=True)
    res = _np.zeros((frames, dfb), dtype=_np.uint8)
    _chk(L.dsv1_rgb_import_clip(device, a.ctypes.data, _C.byref(rf), w, h, fmt, frames, res.ctypes.data, 0), "dsv1_rgb_import_clip")
    return res


def rgb_export_clip(clip, w, h, fmt, rf, device=0, n=None, out=None):
    """packed planar 8-bit frames (w x h at subsampling fmt) to RGB frames of RgbFormat rf on the GPU (dsv1_rgb_export_clip), chroma
    upsampled as rf.upsample says: clip numpy uint8 [frames][frame_bytes] (host), or a device pointer with n frames and `out` a device
    pointer for the result.  Host input returns numpy uint8 [frames][frame bytes of rf]; `out` (a numpy uint8 array of that size) is
    written in place -- what the format pads stays as it was."""
    L = lib()
    sfb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is not None:
        _chk(L.dsv1_rgb_export_clip(device, clip, w, h, fmt, n, out, _C.byref(rf), 1), "dsv1_rgb_export_clip")
        return out
    a, frames = _host_clip(clip, sfb, "a planar clip", raw=True)
    res = _host_out(out, frames, rgb_frame_bytes(rf, w, h))
    _chk(L.dsv1_rgb_export_clip(device, a.ctypes.data, w, h, fmt, frames, res.ctypes.data, _C.byref(rf), 0), "dsv1_rgb_export_clip")
    return res


def hdr_build(hd):
    """the HdrTables of Hdr settings hd (dsv1_hdr_build; host only); ValueError for invalid settings"""
    t = HdrTables()
    if lib().dsv1_hdr_build(_C.byref(hd), _C.byref(t)) != 0:
        raise ValueError("not valid HDR settings")
    return t


def hdr_tables_valid(tables):
    """whether every entry is inside the bounds that keep the pixel path from overflowing (dsv1_hdr_tables_valid)"""
    return bool(lib().dsv1_hdr_tables_valid(_C.byref(tables)))


def hdr_cidx(v):
    """the bucket 0..3328 of a linear value v <= 2^20 (dsv1_hdr_cidx: the header's one text); ValueError above"""
    i = lib().dsv1_hdr_cidx_of(int(v)) if 0 <= int(v) <= HDR_ONE else -1
    if i < 0:
        raise ValueError("no bucket for %r" % (v,))
    return i


def hdr_import_clip(clip, pf, w, h, src_subsamp, fmt, tables, upsample=CHROMA_LINEAR, device=0, n=None, out=None):
    """HDR frames of PixFormat pf (depth 10, 12 or 16) at src_subsamp to packed planar 8-bit SDR Y, Cb, Cr at subsampling fmt on the GPU
    by HdrTables `tables` (dsv1_hdr_import_clip): clip numpy uint8 (host; a whole number of frames, the last one may end with its
    planes), or a device pointer with n frames and `out` a device pointer for the result.  Host input returns numpy uint8
    [frames][planar frame_bytes]."""
    L = lib()
    dfb = w * h + 2 * _chroma_size(w, h, fmt)
    if n is not None:
        _chk(L.dsv1_hdr_import_clip(device, clip, _C.byref(pf), w, h, src_subsamp, fmt, n, out, _C.byref(tables), upsample, 1), "dsv1_hdr_import_clip")
        return out
    a, frames = _host_clip(clip, pix_frame_bytes(pf, w, h, src_subsamp), "a clip of this format", raw=True)
    res = _np.zeros((frames, dfb), dtype=_np.uint8)
    _chk(L.dsv1_hdr_import_clip(device, a.ctypes.data, _C.byref(pf), w, h, src_subsamp, fmt, frames, res.ctypes.data, _C.byref(tables), upsample, 0),
         "dsv1_hdr_import_clip")
    return res


def scale_taps(S, D, filt):
    """taps of one axis of the resampler (dsv1_scale_taps); ValueError outside 1 <= S / D <= 8"""
    t = lib().dsv1_scale_taps(S, D, filt)
    if t < 0:
        raise ValueError("no scale from %d to %d samples with filter %d" % (S, D, filt))
    return t


def scale_weights(S, D, filt):
    """the resampler's weight table of one axis (dsv1_scale_weights, computed on the host): (start int32 [D], q int16 [D, T])"""
    T = scale_taps(S, D, filt)
    start = _np.zeros(D, dtype=_np.int32)
    q = _np.zeros((D, T), dtype=_np.int16)
    _chk(lib().dsv1_scale_weights(S, D, filt, start.ctypes.data, q.ctypes.data, T), "dsv1_scale_weights")
    return start, q


def scale_clip(clip, sw, sh, fmt, dw, dh, filt=SCALE_CUBIC, device=0, n=None, out=None):
    """scale packed planar frames on the GPU (dsv1_scale_clip): clip numpy uint8 [frames][frame_bytes] (host), or a device pointer with
    n frames and `out` a device pointer for the result.  Host input returns numpy uint8 [frames][scaled frame_bytes]."""
    L = lib()
    sfb = sw * sh + 2 * _chroma_size(sw, sh, fmt)
    dfb = dw * dh + 2 * _chroma_size(dw, dh, fmt)
    if n is not None:
        _chk(L.dsv1_scale_clip(device, clip, sw, sh, fmt, n, out, dw, dh, filt, 1), "dsv1_scale_clip")
        return out
    a, frames = _host_clip(clip, sfb, "a clip of %dx%d frames" % (sw, sh))
    res = _np.zeros((frames, dfb), dtype=_np.uint8)
    _chk(L.dsv1_scale_clip(device, a.ctypes.data, sw, sh, fmt, frames, res.ctypes.data, dw, dh, filt, 0), "dsv1_scale_clip")
    return res


def resample_taps(S, D, filt):
    """taps of one axis of the resampler in either direction (dsv1_resample_taps); ValueError outside 1/8 <= S / D <= 8"""
    t = lib().dsv1_resample_taps(S, D, filt)
    if t < 0:
        raise ValueError("no resample from %d to %d samples with filter %d" % (S, D, filt))
    return t


def resample_weights(S, D, filt):
    """the resampler's weight table of one axis, either direction (dsv1_resample_weights): (start int32 [D], q int16 [D, T])"""
    T = resample_taps(S, D, filt)
    start = _np.zeros(D, dtype=_np.int32)
    q = _np.zeros((D, T), dtype=_np.int16)
    _chk(lib().dsv1_resample_weights(S, D, filt, start.ctypes.data, q.ctypes.data, T), "dsv1_resample_weights")
    return start, q


def resample_clip(clip, sw, sh, fmt, dw, dh, filt=SCALE_CUBIC, device=0, n=None, out=None):
    """resample packed planar frames on the GPU, every axis of every plane up or down (dsv1_resample_clip); arguments as scale_clip"""
    L = lib()
    sfb = sw * sh + 2 * _chroma_size(sw, sh, fmt)
    dfb = dw * dh + 2 * _chroma_size(dw, dh, fmt)
    if n is not None:
        _chk(L.dsv1_resample_clip(device, clip, sw, sh, fmt, n, out, dw, dh, filt, 1), "dsv1_resample_clip")
        return out
    a, frames = _host_clip(clip, sfb, "a clip of %dx%d frames" % (sw, sh))
    res = _np.zeros((frames, dfb), dtype=_np.uint8)
    _chk(L.dsv1_resample_clip(device, a.ctypes.data, sw, sh, fmt, frames, res.ctypes.data, dw, dh, filt, 0), "dsv1_resample_clip")
    return res


class ResLadder:
    """A resolution ladder (dsv1_resladder_open): nsources sources of w x h in format fmt, each scaled on the GPU to every geometry of
    `geoms` and coded there at every rate rung.  geoms: list of (width, height, [Encoder cfg of that geometry, ...]).  Input is the
    SOURCE clip [source][frame] (nsources x F frames of w x h: one upload per call); results are per output stream
    k = s * Ntot + off[g] + rate.  sse() / ssim_fx() are against the scaled source of each stream."""

    def __init__(self, w, h, fmt, geoms, nsources, frames_per_call, filt=SCALE_CUBIC, device=0, src_format=None, src_rgb=None,
                 src_subsamp=None, reframe=None, orient=0, src_hdr=None, src_upsample=CHROMA_LINEAR):
        """src_format: the PixFormat of the source clips (dsv1_resladder_open_src; None: packed planar 8-bit); src_rgb: their RgbFormat
        instead (dsv1_resladder_open_rgb); src_subsamp: the subsampling of the source clips where it is not fmt
        (dsv1_resladder_open_src_sub) -- 4:4:4 or 4:2:2, chroma halved to fmt by the converter; reframe: a Reframe of the w x h
        sources (dsv1_resladder_open_reframed), the last pass in front of the scales: its canvas stands for the source from there on
        (self.width x self.height, the rungs' ratio limits, src_psnr / src_ssim), the clips handed in stay w x h; orient: an Orient
        code (dsv1_resladder_open_oriented) applied to the w x h sources in front of the reframe, whose input is then the oriented
        geometry -- without a reframe the oriented picture stands for the source; src_hdr: the HdrTables of an HDR import of
        src_format (depth 10, 12 or 16) at src_subsamp, chroma brought up by src_upsample (dsv1_resladder_open_hdr; not with
        src_rgb, reframe or orient)"""
        if src_hdr is not None and (src_format is None or src_rgb is not None or reframe is not None or orient):
            raise ValueError("src_hdr goes with src_format, and without src_rgb, reframe and orient")
        if src_format is not None and src_rgb is not None:
            raise ValueError("src_format and src_rgb exclude each other")
        if src_subsamp is not None and src_rgb is not None:
            raise ValueError("src_subsamp and src_rgb exclude each other")
        geoms = [(gw, gh, list(rates)) for gw, gh, rates in geoms]
        self.L = lib()
        self.h = _C.c_void_p(None)
        self.width, self.height, self.fmt = w, h, fmt
        self.nsources, self.F = nsources, frames_per_call
        self.geoms = [(gw, gh, len(rates)) for gw, gh, rates in geoms]
        self._arrs = [(Encoder * max(len(r), 1))(*r) for _, _, r in geoms]
        rr = (ResRung * max(len(geoms), 1))(*[ResRung(gw, gh, len(r), a) for (gw, gh, r), a in zip(geoms, self._arrs)])
        meta = Meta()
        meta.width, meta.height, meta.subsamp = w, h, fmt
        if src_hdr is not None:
            _chk(self.L.dsv1_resladder_open_hdr(_C.byref(self.h), _C.byref(meta), _C.byref(src_format), fmt if src_subsamp is None else src_subsamp,
                                                _C.byref(src_hdr), src_upsample, rr, len(geoms), device, nsources, frames_per_call, filt),
                 "dsv1_resladder_open_hdr")
        elif orient:
            _chk(self.L.dsv1_resladder_open_oriented(_C.byref(self.h), _C.byref(meta), orient, None if reframe is None else _C.byref(reframe),
                                                     None if src_format is None else _C.byref(src_format),
                                                     fmt if src_subsamp is None else src_subsamp,
                                                     None if src_rgb is None else _C.byref(src_rgb), rr, len(geoms), device, nsources,
                                                     frames_per_call, filt), "dsv1_resladder_open_oriented")
            self.width, self.height = (reframe.out_w, reframe.out_h) if reframe is not None else orient_dims(orient, w, h)
        elif reframe is not None:
            _chk(self.L.dsv1_resladder_open_reframed(_C.byref(self.h), _C.byref(meta), _C.byref(reframe),
                                                     None if src_format is None else _C.byref(src_format),
                                                     fmt if src_subsamp is None else src_subsamp,
                                                     None if src_rgb is None else _C.byref(src_rgb), rr, len(geoms), device, nsources,
                                                     frames_per_call, filt), "dsv1_resladder_open_reframed")
            self.width, self.height = reframe.out_w, reframe.out_h
        elif src_rgb is not None:
            _chk(self.L.dsv1_resladder_open_rgb(_C.byref(self.h), _C.byref(meta), _C.byref(src_rgb), rr, len(geoms), device, nsources,
                                                frames_per_call, filt), "dsv1_resladder_open_rgb")
        elif src_subsamp is not None:
            _chk(self.L.dsv1_resladder_open_src_sub(_C.byref(self.h), _C.byref(meta), None if src_format is None else _C.byref(src_format),
                                                    src_subsamp, rr, len(geoms), device, nsources, frames_per_call, filt),
                 "dsv1_resladder_open_src_sub")
        elif src_format is None:
            _chk(self.L.dsv1_resladder_open(_C.byref(self.h), _C.byref(meta), rr, len(geoms), device, nsources, frames_per_call, filt),
                 "dsv1_resladder_open")
        else:
            _chk(self.L.dsv1_resladder_open_src(_C.byref(self.h), _C.byref(meta), _C.byref(src_format), rr, len(geoms), device, nsources,
                                                frames_per_call, filt), "dsv1_resladder_open_src")
        self.ntot = sum(n for _, _, n in self.geoms)
        self.nstreams = self.L.dsv1_resladder_nstreams(self.h)
        self.ctx = self.L.dsv1_batch_ctx(self.L.dsv1_resladder_batch(self.h, 0))
        self._dev, self._pin, self._pending = [], [], []

    def stream(self, source, geom, rate):
        """output stream index k of (source, geometry, rate rung)"""
        return source * self.ntot + sum(n for _, _, n in self.geoms[:geom]) + rate

    def stream_dims(self, k):
        """(width, height) of output stream k"""
        o = k % self.ntot
        for gw, gh, n in self.geoms:
            if o < n:
                return gw, gh
            o -= n

    def batch(self, g):
        """geometry g's quality ladder handle (dsv1_resladder_batch)"""
        return self.L.dsv1_resladder_batch(self.h, g)

    def _input(self, yuv):
        a = _np.ascontiguousarray(yuv, dtype=_np.uint8)
        fin = self.in_frames
        if a.size != self.nsources * fin * self.frame_bytes:
            raise ValueError("a resolution ladder call is %d sources x %d frames x %d bytes, got %d bytes" % (
                self.nsources, fin, self.frame_bytes, a.size))
        return a

    _SOURCE_INPUT = "dsv1_resladder_source_input"
    _source_input, in_frames, frame_bytes, in_dims = Batch._source_input, Batch.in_frames, Batch.frame_bytes, Batch.in_dims

    def set_deinterlace(self, di):
        """the sources are interlaced: deinterlace them on the GPU as Deint di says, behind the conversion and in front of the scales
        (dsv1_resladder_set_deinterlace); None switches it off.  Between calls only; contract as Batch.set_source_deinterlace."""
        _chk(self.L.dsv1_resladder_set_deinterlace(self.h, _C.byref(di) if di is not None else None), "dsv1_resladder_set_deinterlace")

    def deinterlace_reset(self, source=-1):
        """a discontinuity in `source` (-1: every source): dsv1_resladder_deinterlace_reset"""
        _chk(self.L.dsv1_resladder_deinterlace_reset(self.h, source), "dsv1_resladder_deinterlace_reset")

    def set_ivtc(self, iv):
        """the sources are 3:2 pulled-down film: inverse telecine them on the GPU as Ivtc iv says, behind the conversion and in front of
        the scales (dsv1_resladder_set_ivtc); None switches it off.  Between calls only; contract as Batch.set_source_ivtc."""
        _chk(self.L.dsv1_resladder_set_ivtc(self.h, _C.byref(iv) if iv is not None else None), "dsv1_resladder_set_ivtc")

    def ivtc_reset(self, source=-1):
        """a discontinuity in `source` (-1: every source): dsv1_resladder_ivtc_reset"""
        _chk(self.L.dsv1_resladder_ivtc_reset(self.h, source), "dsv1_resladder_ivtc_reset")

    def set_levels(self, lv):
        """from the next call on the source clips pass Levels lv on the GPU, directly behind the conversion (dsv1_resladder_set_levels);
        None or the identity switches it off.  The levelled clip stands for the source everywhere behind it, src_psnr / src_ssim
        included.  Between calls only; contract as Batch.set_source_levels."""
        _chk(self.L.dsv1_resladder_set_levels(self.h, _C.byref(lv) if lv is not None else None), "dsv1_resladder_set_levels")

    def set_overlays(self, overlays):
        """from the next call on the Overlay objects of the list are blended onto the source clips on the GPU, on the canvas in front of
        the scales (dsv1_resladder_set_overlays); None or an empty list switches it off.  The overlaid clip stands for the source
        everywhere behind it, src_psnr / src_ssim included.  Between calls only; contract as Batch.set_source_overlays."""
        arr, n = _overlay_array(overlays)
        _chk(self.L.dsv1_resladder_set_overlays(self.h, arr, n), "dsv1_resladder_set_overlays")

    def overlay_seek(self, source, t):
        """the next picture of `source` (-1: every source) is picture t of the overlays' clock (dsv1_resladder_overlay_seek)"""
        _chk(self.L.dsv1_resladder_overlay_seek(self.h, source, t), "dsv1_resladder_overlay_seek")

    def set_denoise(self, dn):
        """the sources pass the temporal noise filter on the GPU as Denoise dn says, behind the conversion and the deinterlacer and in
        front of the scales (dsv1_resladder_set_denoise); None switches it off.  Between calls only; contract as Batch.set_source_denoise."""
        _chk(self.L.dsv1_resladder_set_denoise(self.h, _C.byref(dn) if dn is not None else None), "dsv1_resladder_set_denoise")

    def denoise_reset(self, source=-1):
        """a discontinuity in `source` (-1: every source): dsv1_resladder_denoise_reset"""
        _chk(self.L.dsv1_resladder_denoise_reset(self.h, source), "dsv1_resladder_denoise_reset")

    def _form(self, on_device, held):
        return (2 if held else 1) if on_device else 0

    def encode(self, yuv, on_device=False, eos=False):
        bufs = (Buf * self.nstreams)()
        a = None if on_device else self._input(yuv)
        _chk(self.L.dsv1_resladder_encode(self.h, yuv if on_device else a.ctypes.data, self._form(on_device, False), bufs),
             "dsv1_resladder_encode")
        if eos:
            for k in range(self.nstreams):
                _chk(self.L.dsv1_resladder_eos(self.h, k, _C.byref(bufs[k])), "dsv1_resladder_eos")
        return [_take(bufs[k]) for k in range(self.nstreams)]

    def submit(self, yuv, on_device=False, held=False):
        """enqueue one call (at most two in flight: submit(i+1); collect(i)); device clips as Batch.submit"""
        a = None if on_device else self._input(yuv)
        bufs = (Buf * self.nstreams)()
        _chk(self.L.dsv1_resladder_submit(self.h, yuv if on_device else a.ctypes.data, self._form(on_device, held), bufs),
             "dsv1_resladder_submit")
        self._pending.append((bufs, a))

    def collect(self):
        bufs, _ = self._pending.pop(0)
        _chk(self.L.dsv1_resladder_collect(self.h, bufs), "dsv1_resladder_collect")
        return [_take(bufs[k]) for k in range(self.nstreams)]

    def eos(self, k):
        b = Buf()
        _chk(self.L.dsv1_resladder_eos(self.h, k, _C.byref(b)), "dsv1_resladder_eos")
        return _take(b)

    def encoder(self, k):
        p = self.L.dsv1_resladder_encoder(self.h, k)
        if not p:
            raise IndexError("no stream %d" % k)
        return Encoder.from_address(p)

    def sse_enable(self, on=True):
        _chk(self.L.dsv1_resladder_sse_enable(self.h, 1 if on else 0), "dsv1_resladder_sse_enable")

    def ssim_enable(self, on=True):
        _chk(self.L.dsv1_resladder_ssim_enable(self.h, 1 if on else 0), "dsv1_resladder_ssim_enable")

    def sse(self):
        """numpy.uint64 [nstreams, F, 3] of the call collected last (against each stream's scaled source)"""
        return _figures(self.L.dsv1_resladder_get_sse, self.h, (self.nstreams, self.F, 3), _np.uint64)

    def ssim_fx(self):
        """numpy.int64 [nstreams, F, 3] of the call collected last (against each stream's scaled source)"""
        return _figures(self.L.dsv1_resladder_get_ssim, self.h, (self.nstreams, self.F, 3), _np.int64)

    def psnr(self):
        """float64 [nstreams, F, 4] in dB, each stream at its own geometry"""
        e = self.sse()
        return _np.stack([psnr_db(e[k], *self.stream_dims(k), self.fmt) for k in range(self.nstreams)])

    def ssim(self):
        """mean SSIM float64 [nstreams, F, 4], each stream at its own geometry"""
        f = self.ssim_fx()
        return _np.stack([ssim_mean(f[k], *self.stream_dims(k), self.fmt) for k in range(self.nstreams)])

    def src_quality_enable(self, sse=True, ssim=True, filt=SCALE_CUBIC):
        """measure every rung at the SOURCE resolution (dsv1_resladder_src_quality_enable): reconstructions upscaled with filter
        `filt` and compared with the original source; only between calls"""
        _chk(self.L.dsv1_resladder_src_quality_enable(self.h, 1 if sse else 0, 1 if ssim else 0, filt), "dsv1_resladder_src_quality_enable")

    def src_sse(self):
        """numpy.uint64 [nstreams, F, 3] of the call collected last, over the source's plane areas"""
        return _figures(self.L.dsv1_resladder_get_src_sse, self.h, (self.nstreams, self.F, 3), _np.uint64)

    def src_ssim_fx(self):
        """numpy.int64 [nstreams, F, 3]: SSIM_FX over the windows of the source's plane dims"""
        return _figures(self.L.dsv1_resladder_get_src_ssim, self.h, (self.nstreams, self.F, 3), _np.int64)

    def src_psnr(self):
        """float64 [nstreams, F, 4] in dB, every stream at the source geometry"""
        return psnr_db(self.src_sse(), self.width, self.height, self.fmt)

    def src_ssim(self):
        """mean SSIM float64 [nstreams, F, 4], every stream over the source geometry's windows"""
        return ssim_mean(self.src_ssim_fx(), self.width, self.height, self.fmt)

    def code_streams(self, n=0):
        """set (n >= 1) / query (n = 0) the coding streams of every geometry's ladder; returns the previous value of geometry 0's"""
        prev = [self.L.dsvg_ctx_code_streams(self.L.dsv1_batch_ctx(self.batch(g)), n) for g in range(len(self.geoms))]
        return prev[0]

    def uploads(self):
        """(bytes, calls) the resladder uploaded itself (host input: one source clip per call)"""
        b, c = _C.c_uint64(0), _C.c_long(0)
        _chk(self.L.dsv1_resladder_uploads(self.h, _C.byref(b), _C.byref(c)), "dsv1_resladder_uploads")
        return b.value, c.value

    def upload(self, clip):
        """a raw source clip resident in HBM (device pointer)"""
        return Batch.upload(self, clip)

    def pinned(self, shape):
        return Batch.pinned(self, shape)

    def close(self):
        if self.h:
            self.L.dsvg_ctx_sync(self.ctx)
            for p in self._dev:
                self.L.dsvg_dev_free(self.ctx, p)
            self._dev = []
            for p in self._pin:
                self.L.dsvg_host_free(self.ctx, p)
            self._pin = []
            self.L.dsv1_resladder_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecBatch:
    """nstreams independent streams of one geometry, one packet per stream per decode() call (dsv1_decbatch_*)"""

    def __init__(self, w, h, fmt, nstreams, device=0):
        self.L = lib()
        self.h = _C.c_void_p(None)
        self.nstreams = nstreams
        self.fmt = fmt
        m = Meta()
        m.width, m.height, m.subsamp = w, h, fmt
        _chk(self.L.dsv1_decbatch_open(_C.byref(self.h), device, _C.byref(m), nstreams), "dsv1_decbatch_open")
        self.frame_bytes = w * h + 2 * _chroma_size(w, h, fmt)
        self._dev = None

    @property
    def ctx(self):
        """the device context (not cached: the batch builds a new one when its streams announce another block size)"""
        return self.L.dsv1_decbatch_ctx(self.h)

    def mem_live(self):
        """{buffer name: bytes} the batch's device context holds now (ctx_mem_live)"""
        return ctx_mem_live(self.ctx)

    def _output_changed(self):
        self.frame_bytes = int(self.L.dsv1_decbatch_out_frame_bytes(self.h))
        if self._dev is not None:                      # (sized for the frames of the setting before)
            self.sync()
            self.L.dsvg_dev_free(self.ctx, self._dev)
            self._dev = None

    def set_output_format(self, pixformat, out_subsamp=None, upsample=None):
        """from the next decode() on, frames are written as PixFormat pixformat at subsampling out_subsamp (None: the streams' own;
        dsv1_decbatch_set_output_format); None switches back to packed planar.  frame_bytes follows; ValueError (and the setting as
        it was) for an invalid combination.  upsample (CHROMA_REPLICATE / CHROMA_LINEAR; dsv1_decbatch_set_output_format_up):
        out_subsamp may also be a finer one than the streams', chroma doubled that way."""
        osub = self.fmt if out_subsamp is None else out_subsamp
        pfp = None if pixformat is None else _C.byref(pixformat)
        if upsample is None:
            rc = self.L.dsv1_decbatch_set_output_format(self.h, pfp, osub)
        else:
            rc = self.L.dsv1_decbatch_set_output_format_up(self.h, pfp, osub, upsample)
        if rc != 0:
            raise ValueError("not a valid output format for these streams (subsampling 0x%x -> 0x%x)" % (self.fmt, osub))
        self._output_changed()

    def set_output_rgb(self, rf):
        """from the next decode() on, frames are written as RGB of RgbFormat rf (dsv1_decbatch_set_output_rgb); None switches back to
        packed planar.  Replaces an output format set before.  frame_bytes follows; ValueError (and the setting as it was) for an
        invalid format."""
        if self.L.dsv1_decbatch_set_output_rgb(self.h, None if rf is None else _C.byref(rf)) != 0:
            raise ValueError("not a valid RGB output format for these streams (subsampling 0x%x)" % self.fmt)
        self._output_changed()

    def set_output_scale(self, w, h=None, filt=SCALE_CUBIC):
        """from the next decode() on, frames are handed out at w x h in the place of the streams' size, resampled in the output pass
        (dsv1_decbatch_set_output_scale; filt: SCALE_TENT / SCALE_CUBIC); None or 0, 0 switches it off.  Scale first, format second:
        the call drops the output format in force (packed planar frames of the scaled geometry again), and set_output_format /
        set_output_rgb called after it resolve for w x h.  frame_bytes and out_dims follow; ValueError (and scale and format as
        they were) for a ratio outside 1/8 .. 8 on an axis of a plane, a size that is not positive or an unknown filter."""
        if w is None:
            w, h = 0, 0
        if self.L.dsv1_decbatch_set_output_scale(self.h, int(w), int(0 if h is None else h), int(filt)) != 0:
            raise ValueError("not a valid output scale for these streams: %r x %r, filter %r" % (w, h, filt))
        self._output_changed()

    @property
    def out_dims(self):
        """(w, h) of the luma plane of the frames handed out under the setting in force (dsv1_decbatch_out_dims)"""
        w, h = _C.c_int(0), _C.c_int(0)
        _chk(self.L.dsv1_decbatch_out_dims(self.h, _C.byref(w), _C.byref(h)), "dsv1_decbatch_out_dims")
        return w.value, h.value

    def set_draw_info(self, mode):
        """from the next decode() on, the debug overlay of mode 0 .. 7 (DSV_DRAW_* bits; 0: off) is drawn onto the luma of every picture
        that has a reference, ahead of the output pass (dsv1_decbatch_set_draw_info); ValueError for another mode."""
        if self.L.dsv1_decbatch_set_draw_info(self.h, mode) != 0:
            raise ValueError("not a draw_info mode: %r" % (mode,))

    def decode(self, packets, out=None, on_device=False):
        """packets: one bytes object per stream.  Host output: returns (frames [nstreams][frame_bytes] uint8, status,
        fnum); on_device=True leaves the frames in a device buffer owned by this object (returns its pointer)."""
        S = self.nstreams
        assert len(packets) == S
        keep = [_np.frombuffer(bytes(p) + b"\0" * 16, dtype=_np.uint8).copy() for p in packets]
        bufs = (Buf * S)()
        for s in range(S):
            bufs[s].data = keep[s].ctypes.data_as(_C.POINTER(_C.c_uint8))
            bufs[s].len = len(packets[s])
        status = (_C.c_int * S)()
        fnum = (_C.c_uint32 * S)()
        if on_device and out is not None:
            dst = out                                  # a device buffer of the caller's (nstreams x frame_bytes: dev_alloc())
        elif on_device:
            if self._dev is None:
                self._dev = _C.c_void_p(None)
                _chk(self.L.dsvg_dev_alloc(self.ctx, _C.byref(self._dev), self.frame_bytes * S), "dsvg_dev_alloc")
            dst = self._dev
        else:
            if out is None:
                out = _np.zeros((S, self.frame_bytes), dtype=_np.uint8)
            dst = out.ctypes.data
        _chk(self.L.dsv1_decbatch_decode(self.h, bufs, dst, self.frame_bytes, 1 if on_device else 0, status, fnum), "dsv1_decbatch_decode")
        return (dst if on_device else out), list(status), list(fnum)

    def sync(self):
        _chk(self.L.dsvg_ctx_sync(self.ctx), "dsvg_ctx_sync")

    def dev_alloc(self):
        """a device buffer for one call's frames (decode(.., out=buffer, on_device=True)); freed with the context"""
        p = _C.c_void_p(None)
        _chk(self.L.dsvg_dev_alloc(self.ctx, _C.byref(p), self.frame_bytes * self.nstreams), "dsvg_dev_alloc")
        return p

    def download(self, dev=None):
        """host copy of the device output buffer of the last decode(on_device=True), or of `dev`"""
        self.sync()
        out = _np.zeros((self.nstreams, self.frame_bytes), dtype=_np.uint8)
        _chk(self.L.dsvg_dev_download(self.ctx, out.ctypes.data, dev if dev is not None else self._dev, out.nbytes), "dsvg_dev_download")
        return out

    def close(self):
        if self.h:
            self.L.dsvg_ctx_sync(self.ctx)
            if self._dev is not None:
                self.L.dsvg_dev_free(self.ctx, self._dev)
                self._dev = None
            self.L.dsv1_decbatch_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _chroma_size(w, h, fmt):
    """chroma plane samples for a DSV_SUBSAMP_* format code (dsv.h:62-75: bits 2-3 horizontal, 0-1 vertical shift)"""
    hs, vs = (fmt >> 2) & 3, fmt & 3
    return ((w + (1 << hs) - 1) >> hs) * ((h + (1 << vs) - 1) >> vs)


def plane_samples(w, h, fmt):
    """samples of the planes Y, U, V of a w x h picture in DSV_SUBSAMP_* format fmt (chroma rounded up, as the codec sizes it)"""
    c = _chroma_size(w, h, fmt)
    return w * h, c, c


def _figures(getter, handle, shape, dtype):
    """one kind of quality figure of the batch or call collected last (handle: a Batch's, a ResLadder's) through the library's getter
    for it -> numpy array of that shape and dtype (SSE uint64, SSIM_FX int64).  Raises if it was not measured."""
    out = _np.zeros(shape, dtype=dtype)
    _chk(getter(handle, out.ctypes.data_as(_C.POINTER(_np.ctypeslib.as_ctypes_type(dtype))), out.size), getter.__name__)
    return out


def psnr_db(sse, w, h, fmt):
    """PSNR in dB from per-plane sums of squared errors (any array whose last axis is Y, U, V) of w x h pictures in format fmt:
    float64 array with the last axis Y, U, V, whole picture -- 10 log10(255^2 N / SSE) per plane and sum SSE / sum N over the
    picture; inf where the SSE is 0"""
    e = _np.asarray(sse, dtype=_np.uint64)
    if e.shape[-1:] != (3,):
        raise ValueError("the last axis of sse must hold the three planes")
    n = _np.array(plane_samples(w, h, fmt), dtype=_np.float64)
    num = _np.concatenate([_np.broadcast_to(n, e.shape), _np.full(e.shape[:-1] + (1,), n.sum())], axis=-1) * (255.0 * 255.0)
    den = _np.concatenate([e, e.sum(axis=-1, dtype=_np.uint64, keepdims=True)], axis=-1).astype(_np.float64)
    with _np.errstate(divide="ignore"):
        return _np.where(den == 0, _np.inf, 10.0 * _np.log10(num / _np.where(den == 0, 1.0, den)))


SSIM_ONE = 1 << 32   # DSVG_SSIM_ONE: the fixed-point scale of one window's SSIM


def ssim_windows(w, h, fmt):
    """8x8 SSIM windows at stride 4 of the planes Y, U, V of a w x h picture in format fmt: ((pw - 8) // 4 + 1) * ((ph - 8) // 4 + 1)
    per plane of pw x ph samples (chroma at its subsampled size), 0 where the plane is narrower or shorter than 8"""
    hs, vs = (fmt >> 2) & 3, fmt & 3
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs

    def n(pw, ph):
        return ((pw - 8) // 4 + 1) * ((ph - 8) // 4 + 1) if pw >= 8 and ph >= 8 else 0
    return n(w, h), n(cw, ch), n(cw, ch)


def ssim_mean(fx, w, h, fmt):
    """mean SSIM from fixed-point per-plane sums (any array whose last axis is Y, U, V; Batch.ssim_fx()) of w x h pictures in format
    fmt: float64 array with the last axis Y, U, V, whole picture -- fx / (2^32 nwin) per plane and sum fx / (2^32 sum nwin) over
    the picture; NaN where there is no window"""
    f = _np.asarray(fx, dtype=_np.int64)
    if f.shape[-1:] != (3,):
        raise ValueError("the last axis of fx must hold the three planes")
    n = _np.array(ssim_windows(w, h, fmt), dtype=_np.float64)
    num = _np.concatenate([f, f.sum(axis=-1, keepdims=True)], axis=-1).astype(_np.float64)
    den = _np.concatenate([_np.broadcast_to(n, f.shape), _np.full(f.shape[:-1] + (1,), n.sum())], axis=-1) * float(SSIM_ONE)
    with _np.errstate(divide="ignore", invalid="ignore"):
        return _np.where(den == 0, _np.nan, num / _np.where(den == 0, 1.0, den))


def ssim_db(x):
    """SSIM in dB: -10 log10(1 - x), +inf at 1 (float64, elementwise)"""
    x = _np.asarray(x, dtype=_np.float64)
    with _np.errstate(divide="ignore"):
        return -10.0 * _np.log10(1.0 - x)


def encode_clip(clip, w, h, fmt, device=0, eos=True, start_fnum=0, **cli):
    """one serial stream on the GPU: the whole clip in one batch call -> .dsv bytes"""
    cfg = make_encoder_cfg(w, h, fmt, **cli)
    n = clip.shape[0]
    b = Batch(cfg, 1, n, device)
    try:
        if start_fnum:
            b.set_fnum(0, start_fnum)
        return b.encode(clip.reshape(1, n, -1), eos=eos)[0]
    finally:
        b.close()


def encode_stream(clip, w, h, fmt, frames_per_call, chains, device=0, eos=True, **cli):
    """one stream through the GOP-parallel chain mode (dsv1_stream_open): the clip in calls of frames_per_call frames
    (clip.shape[0] must be a multiple), two calls in flight -> .dsv bytes, byte for byte the serial encoder's"""
    cfg = make_encoder_cfg(w, h, fmt, **cli)
    n = clip.shape[0]
    assert n % frames_per_call == 0
    b = Batch(cfg, 1, frames_per_call, device, chains=chains)
    try:
        out = b""
        calls = [clip[i:i + frames_per_call].reshape(1, frames_per_call, -1) for i in range(0, n, frames_per_call)]
        b.submit(calls[0])
        for k in range(1, len(calls)):
            b.submit(calls[k])
            out += bytes(b.collect()[0])
        out += bytes(b.collect()[0])
        if eos:
            e = Buf()
            _chk(b.L.dsv1_batch_eos(b.h, 0, _C.byref(e)), "dsv1_batch_eos")
            out += _take(e)
        return out
    finally:
        b.close()


def encode_ladder(clip, w, h, fmt, rungs, device=0, eos=True, **cli):
    """one source coded at several rungs in one call (a Ladder of one source): clip [frames][frame_bytes]; rungs: a list of dicts of
    make_encoder_cfg arguments that override `cli` per rung (e.g. [dict(qp=95), dict(qp=70)]) -> one .dsv bytes object per rung,
    each byte for byte the stream the serial encoder writes with that rung's settings"""
    n = clip.shape[0]
    b = Ladder([make_encoder_cfg(w, h, fmt, **dict(cli, **r)) for r in rungs], 1, n, device)
    try:
        return b.encode(clip.reshape(1, n, -1), eos=eos)
    finally:
        b.close()


def encode_resolution_ladder(clip, w, h, fmt, rungs, filt=SCALE_CUBIC, device=0, eos=True, **cli):
    """one source coded at several geometries and rates in one call: clip [frames][frame_bytes] of w x h; rungs: a list of
    dict(w=, h=, rates=[dict of make_encoder_cfg arguments overriding `cli`, ...]) -> one .dsv bytes object per (geometry, rate), in
    that order, each the stream the serial encoder writes for the clip scaled to that geometry (scale_clip)"""
    n = clip.shape[0]
    geoms = [(r["w"], r["h"], [make_encoder_cfg(r["w"], r["h"], fmt, **dict(cli, **q)) for q in r["rates"]]) for r in rungs]
    b = ResLadder(w, h, fmt, geoms, 1, n, filt, device)
    try:
        return b.encode(clip.reshape(1, n, -1), eos=eos)
    finally:
        b.close()


def concat_gops(streams):
    """join independently encoded closed GOPs exactly as one serial encode would have linked them"""
    L = lib()
    arr = (Buf * len(streams))()
    keep = []
    for i, s in enumerate(streams):
        a = _np.frombuffer(s, dtype=_np.uint8).copy()
        keep.append(a)
        arr[i].data = a.ctypes.data_as(_C.POINTER(_C.c_uint8))
        arr[i].len = a.size
    out = Buf()
    _chk(L.dsv1_concat_gops(arr, len(streams), _C.byref(out)), "dsv1_concat_gops")
    return _take(out)


def encode_gops(clip, w, h, fmt, gop, device=0, **cli):
    """GOP-sharded encode: clip (N frames, N % gop == 0) -> N/gop independent closed GOPs in ONE batch,
    each seeded with its frame number, then joined.  Bit-exact with the serial stream when GOPs are
    independent (CRF, stable_refresh == gop-1, no forced-intra P frames: SURVEY.md 8e)."""
    n = clip.shape[0]
    assert n % gop == 0
    g = n // gop
    cfg = make_encoder_cfg(w, h, fmt, gop=gop, **cli)
    b = Batch(cfg, g, gop, device)
    try:
        for s in range(g):
            b.set_fnum(s, s * gop)
        parts = b.encode(clip.reshape(g, gop, -1))
    finally:
        b.close()
    return concat_gops(parts)
