"""GPU parity of batches of previews: ipk_pipeline_run_batch under IPK_FUSED_BATCH_PREVIEWS (allow_fused bit 8), the batch mode of
k_raw_scaled_demosaic<uint16_t | float> behind it (blockIdx.z = the frame, the launch log's batch=1), and the primitives ipk_raw_scaled_demosaic_batch /
ipk_plain_scale_down_batch.  Bar: bit-exact (f32 bit patterns, any NaN == any NaN; equal u8 / u16) against the CPU oracle's pipeline per frame and against
ipk_pipeline_run per frame.  Every frame of a batch has its own seed, so a mixed-up frame index cannot pass; every destination lies between guard bands;
sources are views at odd element offsets of one poisoned allocation.  Sizes and branches are asserted from ipk_pipeline_sizes and the route report."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_batch_previews_route as br
from test_batch_previews_route import XT, ON, PLAIN_PREVIEWS, BATCH, OUT_F32, OUT_U8, OUT_U16

pytestmark = pytest.mark.gpu

NP_OUT = {OUT_F32: np.dtype(np.float32), OUT_U8: np.dtype(np.uint8), OUT_U16: np.dtype(np.uint16)}
SRC_TYPE = {"u16": br.U16, "f32": br.F32, "rgb8": br.RGB8}
CTYPE = {"u16": "unsigned short", "f32": "float"}
S1 = "batch gofloat+demosaic"
S2 = {OUT_F32: "batch to_lab+basecurve+from_lab+gamma", OUT_U8: "batch to_lab+basecurve+from_lab+gamma+quantise",
      OUT_U16: "batch to_lab+basecurve+from_lab+gamma+quantise"}
B3, W3 = (64.0, 128.0, 256.0, 0.0), (1023.0, 4095.0, 16383.0, 0.0)       # a three-sample raw's levels: different per channel
B3D, W3D = (64.0, 300.0, 256.0, 0.0), (1023.0, 300.0, 16383.0, 0.0)      # ... with one degenerate pair: channel 1 has a range of 0


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


class Spec:
    """one kind of frame and its descriptor: w x h sensor samples (kind: a filter string, "mono", "cpp3" or "rgb8"), sensor crops, the size limit"""

    def __init__(self, kind, src, w, h, maxwidth, crops=(0, 0, 0, 0), levels=None, mask=ON | BATCH, **ops):
        self.kind, self.src, self.w, self.h, self.maxwidth, self.crops, self.mask, self.ops = kind, src, w, h, maxwidth, crops, mask, ops
        self.cfa = kind if kind not in ("mono", "cpp3", "rgb8") else ""
        self.cpp = 1 if self.cfa or kind == "mono" else 3
        self.levels = levels or ((B3, W3) if kind == "cpp3" else ([util.BLACK] * 4, [util.WHITE] * 4))

    def shifted(self, L):
        if not self.cfa:
            return ""
        out = C.create_string_buffer(160)
        assert L.ipk_cfa_shift(self.cfa.encode(), self.crops[3], self.crops[0], out) == 0
        return out.value.decode()

    def desc(self, L, out, linear=0, mask=None):
        kw = dict(self.ops)
        if "rotatecrop" in kw:
            kw["rotatecrop"] = [float(np.float32(v)) for v in kw["rotatecrop"]]
        if self.kind == "rgb8":
            kw["exposure"] = 0.25                                           # not the default ops: no fast path
        return br.make_desc(self.w, self.h, self.shifted(L), self.crops, src_type=SRC_TYPE[self.src], cpp=self.cpp, is_cfa=int(bool(self.cfa)),
                            allow_fused=self.mask if mask is None else mask, maxwidth=self.maxwidth, linear=linear,
                            blacklevels=list(self.levels[0]), whitelevels=list(self.levels[1]), **kw)

    def frame(self, seed, specials=False):
        spp = 3 if self.kind in ("cpp3", "rgb8") else 1
        if self.kind == "rgb8":
            return (util.splitmix64(seed, self.h * self.w * 3) & np.uint64(255)).astype(np.uint8).reshape(self.h, self.w, 3)
        data = util.noise_u16(seed, self.h, self.w * spp, 18000)
        if self.src == "f32":
            data = data.astype(np.float32) + util.uniform_f32(seed + 1, data.size, -0.5, 0.5).reshape(data.shape)
            if specials:                                                   # the suite's special values, scaled to the white level, inside the crop window
                with np.errstate(over="ignore"):
                    spc = util.SPECIALS * np.float32(16383.0)
                t, r, b, l = self.crops
                row = (self.w - l - r) * spp
                for k in range(0, spc.size, row):
                    part = spc[k: k + row]
                    data[t + 1 + 2 * (k // row), l * spp: l * spp + part.size] = part
                data[t + self.h // 2, (l + self.w // 3) * spp] = -np.inf
                data[self.h - b - 2, (l + 3) * spp + spp - 1] = np.nan
                data[t + 5, (self.w - r - 2) * spp] = np.inf
        return data.reshape(self.h, self.w, 3) if spp == 3 else data

    def oracle(self, orc, L, data, out, linear=0):
        ops = dict(self.ops)
        if self.kind == "rgb8":
            ops["exposure"] = 0.25
        desc = orc.make_pipeline(data, cfa=self.shifted(L), is_cfa=bool(self.cfa), cpp=self.cpp, crops=self.crops, blacklevels=self.levels[0],
                                 whitelevels=self.levels[1], cam_to_xyz_normalized=util.cam_matrix(), wb_coeffs=util.WB, points=[(0.5, 0.6)],
                                 maxwidth=self.maxwidth, linear=bool(linear), **ops)
        threads = orc.max_threads()
        if self.w * self.h < 1 << 18:
            orc.set_num_threads(1)                                          # a thumbnail's source: starting a team of threads costs more than the frame
        try:
            with np.errstate(all="ignore"):
                return {OUT_F32: orc.pipeline_run, OUT_U8: orc.pipeline_output_8bit, OUT_U16: orc.pipeline_output_16bit}[out](desc)
        finally:
            orc.set_num_threads(threads)


class Frames:
    """n host frames, each from its own seed, and their device copies: views at odd element offsets of ONE allocation with poison between them (a u16
    frame starts two bytes off a dword boundary)"""

    def __init__(self, spec, n, seed, specials_in=1, derive=False):
        import torch
        if derive:                                                          # large frames: one noise field, every frame a different shift of it modulo 2^14
            base = spec.frame(seed).astype(np.uint32)
            self.host = [((base + 977 * i) % 16384).astype(np.uint16) for i in range(n)]
        else:
            self.host = [spec.frame(seed + 7919 * i, specials=(i == specials_in)) for i in range(n)]
        size = self.host[0].size
        step = size + (1 if size % 2 else 2)                                # even: every frame starts at an odd element
        dt = self.host[0].dtype
        if dt == np.uint8:
            all_ = np.full(1 + n * step, 0x5A, np.uint8)
        else:
            all_ = np.full(1 + n * step, util.POISONS[dt.name], np.dtype("uint32" if dt == np.float32 else "uint16")).view(dt)
        for i, f in enumerate(self.host):
            all_[1 + i * step: 1 + i * step + size] = f.ravel()
        self.t = torch.from_numpy(all_.view(np.int16) if dt == np.uint16 else all_).cuda()
        self.ptrs = [self.t.data_ptr() + (1 + i * step) * self.t.element_size() for i in range(n)]
        self.views = [self.t[1 + i * step: 1 + i * step + size] for i in range(n)]
        assert all((p // self.t.element_size()) % 2 == 1 for p in self.ptrs)


def _stage_names(L, run):
    from imagepipe_amd import _lib
    _lib.check(L.ipk_timing_begin(), "ipk_timing_begin")
    try:
        run()
    finally:
        arr = (_lib.StageTime * 256)()
        n = C.c_int(0)
        _lib.check(L.ipk_timing_end(arr, 256, C.byref(n)), "ipk_timing_end")
    assert n.value <= 256
    return [arr[i].name.decode() for i in range(n.value)]


def run_batch(ipa, d, ptrs, out, px3, slots=None, multi=False):
    """ipk_pipeline_run_batch into one guarded allocation: frame i in slot slots[i] (default i, so the destinations follow each other).
    -> (the allocation's interior as [slot, px3], the launch log, the stage names, used_fused)"""
    import torch
    L = ipa.lib()
    n = len(ptrs)
    slots = list(range(n)) if slots is None else slots
    g = util.Guarded((max(slots) + 1) * px3, NP_OUT[out], off=1)
    esz = NP_OUT[out].itemsize
    sp = (C.c_void_p * n)(*ptrs)
    dp = (C.c_void_p * n)(*[g.ptr + s * px3 * esz for s in slots])
    used = C.c_int(-1)

    def call():
        if multi:
            assert L.ipk_pipeline_run_batch_multi(C.byref(d), sp, dp, n, out, C.byref(used)) == 0, L.ipk_last_error()
            assert L.ipk_devices_sync() == 0
        else:
            assert L.ipk_pipeline_run_batch(C.byref(d), sp, dp, n, out, C.byref(used), ipa._stream()) == 0, L.ipk_last_error()
            torch.cuda.synchronize()
    with ipa.launch_log() as ran:
        names = _stage_names(L, call)
    return g.result("batch of %d" % n).reshape(max(slots) + 1, px3), ran, names, used.value


def run_singles(ipa, d, ptrs, out, px3):
    """ipk_pipeline_run frame by frame, with the descriptor's mask as it is -> ([n, px3], the launch log, the stage names of frame 0, used_fused)"""
    import torch
    L = ipa.lib()
    n = len(ptrs)
    g = util.Guarded(n * px3, NP_OUT[out], off=3)
    used = C.c_int(-1)
    names = None
    with ipa.launch_log() as ran:
        for i, p in enumerate(ptrs):
            def call():
                assert L.ipk_pipeline_run(C.byref(d), p, g.ptr + i * px3 * NP_OUT[out].itemsize, out, C.byref(used), ipa._stream()) == 0, L.ipk_last_error()
            if i == 0:
                names = _stage_names(L, call)
            else:
                call()
        torch.cuda.synchronize()
    return g.result("singles").reshape(n, px3), ran, names, used.value


def same(got, want, what):
    if want.dtype == np.float32:
        util.assert_bits_equal(got, want.ravel(), what)
    else:
        assert got.shape == want.ravel().shape and np.array_equal(got, want.ravel()), "%s: %d samples differ" % (what, int((got != want.ravel()).sum()))


def batch_entries(ran):
    return sorted(e for e in ran if "batch=1" in e)


def check_route(ipa, orc, spec, frames, n, out, linear=0, want_p1=1, tag_re=None, oracle_frames=None, wants=None):
    """the batch with the bit against the oracle, against ipk_pipeline_run per frame and against the batch without the bit; the log and the stages"""
    L = ipa.lib()
    d = spec.desc(L, out, linear)
    dw, dh, fw, fh = br.sizes(L, d)
    assert (dw, dh) == (fw, fh) and dw * dh >= 256
    px3 = fw * fh * 3
    taken, chunk, p1 = br.report(L, d, n, out)
    assert (taken, chunk, p1) == (1, br.chunk_of(dw, dh), want_p1), (spec.kind, n, taken, chunk, p1)
    tag = "%s %s %dx%d -> %dx%d, n = %d, out %d, linear %d" % (spec.kind[:4], spec.src, spec.w, spec.h, dw, dh, n, out, linear)
    ptrs = frames.ptrs[:n]
    got, ran, names, used = run_batch(ipa, d, ptrs, out, px3)
    singles, ran1, names1, used1 = run_singles(ipa, d, ptrs, out, px3)
    assert used == used1 == 0, tag
    for i in (range(n) if oracle_frames is None else oracle_frames):
        want = wants[i] if wants is not None else spec.oracle(orc, L, frames.host[i], out, linear)
        assert want.shape == (fh, fw, 3), tag
        same(got[i], want, "%s: frame %d against the oracle" % (tag, i))
    for i in range(n):
        same(got[i], singles[i], "%s: frame %d against ipk_pipeline_run" % (tag, i))
    # the log and the stages: pass 1 as one batch launch (or the frame's own kernel per frame), two stages per chunk of more than one frame
    full, rest = divmod(n, chunk)
    multi_chunks = full + (1 if rest > 1 else 0)
    if want_p1:
        hits = [e for e in ran if re.match(tag_re, e)]
        assert len(hits) == 1 and batch_entries(ran) == hits, (tag, sorted(ran))
    else:
        assert not batch_entries(ran), (tag, sorted(ran))
        assert [e for e in ran if re.match(tag_re, e)], (tag, sorted(ran))
    assert names.count(S1) == multi_chunks and names.count(S2[out]) == multi_chunks, (tag, names)
    if rest != 1:
        assert len(names) == 2 * multi_chunks, (tag, names)
    else:
        assert names[2 * multi_chunks:] == names1, (tag, names, names1)    # a chunk of one frame is ipk_pipeline_run
    assert not batch_entries(ran1) and not [s for s in names1 if s.startswith("batch")], (tag, sorted(ran1), names1)
    # without the bit: the loop, the same bits
    d0 = spec.desc(L, out, linear, mask=spec.mask & ~BATCH)
    assert br.report(L, d0, n, out) == (0, 0, 0)
    got0, ran0, names0, used0 = run_batch(ipa, d0, ptrs, out, px3)
    assert not batch_entries(ran0) and not [s for s in names0 if s.startswith("batch")] and used0 == 0, (tag, sorted(ran0), names0)
    assert names0 == names1 * n, (tag, names0, names1)
    for i in range(n):
        same(got0[i], got[i], "%s: frame %d without the bit" % (tag, i))
    return got


def mosaic_tag(src):
    return r"^ipk::k_raw_scaled_demosaic<%s>\[norm_fast=[01],norm_light=[01],fast_x=[01],fast_y=[01],xcd=0,batch=1\]$" % re.escape(CTYPE[src])


# ---------------------------------------------------------------------------------------------
# 1. the driver on the batch kernel
# ---------------------------------------------------------------------------------------------
# 211x157 RGGB with sensor crops (2, 3, 4, 5) -> 203x151 -> 23x17 = 391 pixels, skip_x about 9.2; X-Trans 300x240 -> 30 wide
MOSAICS = {"rggb": dict(kind="RGGB", w=211, h=157, maxwidth=23, crops=(2, 3, 4, 5)), "xtrans": dict(kind=XT, w=300, h=240, maxwidth=30)}
# (output, linear): f32 with gamma and without; 8 bits (gamma forced on), 16 bits (forced off)
OUTS = [(OUT_F32, 0), (OUT_F32, 1), (OUT_U8, 0), (OUT_U16, 0)]
_FRAMES = {}


def mosaic_frames(name, src):
    """65 frames per mosaic and sample type, built once"""
    if (name, src) not in _FRAMES:
        spec = Spec(src=src, **MOSAICS[name])
        _FRAMES[(name, src)] = (spec, Frames(spec, 65, util.SEED + 20000 + 1000 * len(name) + (src == "f32")))
    return _FRAMES[(name, src)]


def test_the_mosaics_are_what_they_claim(ipa):
    L = ipa.lib()
    f = np.float32
    spec = Spec(src="u16", **MOSAICS["rggb"])
    d = spec.desc(L, OUT_U8)
    assert br.cropped(d) == (203, 151) and br.sizes(L, d)[:2] == (23, 17) and 23 * 17 == 391
    assert 9.1 < float(f(202) / f(22)) < 9.3
    spec = Spec(src="u16", **MOSAICS["xtrans"])
    dw, dh = br.sizes(L, spec.desc(L, OUT_U8))[:2]
    assert dw == 30 and dw * dh >= 256 and float(f(299) / f(dw - 1)) > 7.0


@pytest.mark.parametrize("k", range(16))
def test_driver_small_batches(ipa, orc, k):
    """every mosaic x sample type x output, at n = 2 or 3"""
    name, src = [(m, s) for m in MOSAICS for s in ("u16", "f32")][k // 4]
    out, linear = OUTS[k % 4]
    spec, frames = mosaic_frames(name, src)
    check_route(ipa, orc, spec, frames, 2 + (k + k // 4) % 2, out, linear, tag_re=mosaic_tag(src))


@pytest.mark.parametrize("name,src,n,out,linear", [("rggb", "u16", 64, OUT_U8, 0), ("rggb", "f32", 65, OUT_F32, 0), ("xtrans", "u16", 65, OUT_U16, 0),
                                                   ("xtrans", "f32", 64, OUT_F32, 1)])
def test_driver_full_launches(ipa, orc, name, src, n, out, linear):
    """64 frames fill one launch; 65 cross it into a chunk of one frame, which is ipk_pipeline_run"""
    spec, frames = mosaic_frames(name, src)
    check_route(ipa, orc, spec, frames, n, out, linear, tag_re=mosaic_tag(src))


def test_the_python_wrapper(ipa, orc):
    """Pipeline.run_batch / batches_previews: one (n, h, w, 3) tensor, so the destinations follow each other"""
    import torch
    spec, frames = mosaic_frames("rggb", "u16")
    L = ipa.lib()
    img = ipa.RawImage(width=spec.w, height=spec.h, data=frames.views[0], cfa="RGGB", crops=spec.crops, blacklevels=[util.BLACK] * 4,
                       whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix())
    pipe = ipa.Pipeline.new_from_source(img)
    pipe.globals.settings.maxwidth = spec.maxwidth
    pipe.ops.basecurve.points = [(0.5, 0.6)]
    assert pipe.batches_previews(5, OUT_U8) == (False, 0, False)
    pipe.batch_previews = True
    assert pipe.desc().allow_fused == ON | BATCH == ON | ipa.FUSED_BATCH_PREVIEWS
    assert pipe.batches_previews(5, OUT_U8) == (True, 64, True) and pipe.batches_previews(1, OUT_U8) == (False, 0, False)
    with ipa.launch_log() as ran:
        got = pipe.run_batch(frames.views[:5], OUT_U8)
        torch.cuda.synchronize()
    assert tuple(got.shape) == (5, 17, 23, 3) and got.is_contiguous() and pipe.last_used_fused is False
    assert len(batch_entries(ran)) == 1, sorted(ran)
    got = got.cpu().numpy()
    for i in range(5):
        same(got[i].ravel(), spec.oracle(orc, L, frames.host[i], OUT_U8), "run_batch frame %d" % i)


# ---------------------------------------------------------------------------------------------
# 2. layouts: monochrome and three-sample raws under bit 7
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,src,out,levels", [("mono", "u16", OUT_U8, None), ("mono", "f32", OUT_F32, None), ("cpp3", "u16", OUT_F32, None),
                                                 ("cpp3", "f32", OUT_U16, None), ("cpp3", "u16", OUT_U8, (B3D, W3D))])
def test_layouts(ipa, orc, kind, src, out, levels):
    spec = Spec(kind, src, 131, 113, 30, crops=(3, 1, 2, 5), levels=levels, mask=ON | BATCH | PLAIN_PREVIEWS)
    frames = Frames(spec, 3, util.SEED + 21000 + 10 * len(kind) + (src == "f32") + 100 * bool(levels))
    tag_re = r"^ipk::k_raw_scaled_demosaic<%s>\[norm_fast=0,norm_light=0,fast_x=[01],fast_y=[01],xcd=0,plain=%d,batch=1\]$" % (
        re.escape(CTYPE[src]), 1 if kind == "mono" else 3)
    check_route(ipa, orc, spec, frames, 3, out, tag_re=tag_re)
    # without bit 7 the frames are not on the route at all
    L = ipa.lib()
    assert br.report(L, spec.desc(L, out, mask=ON | BATCH), 3, out) == (0, 0, 0)


# ---------------------------------------------------------------------------------------------
# 3. pass 1 frame by frame: the window-8 kernel and the raster scaler have no batch form
# ---------------------------------------------------------------------------------------------
def test_pass1_per_frame_w8m(ipa, orc):
    L = ipa.lib()
    spec = Spec(XT, "u16", 300, 200, 75)                                    # skips of 4.0: above X-Trans's minscale of 3, inside the window-8 kernel's 1..7
    assert br.sizes(L, spec.desc(L, OUT_U8))[:2] == (75, 50)
    frames = Frames(spec, 3, util.SEED + 22000)
    for out in (OUT_U8, OUT_F32):
        check_route(ipa, orc, spec, frames, 3, out, want_p1=0, tag_re=r"^ipk::k_raw_scaled_demosaic_w8m<unsigned short, [235]u, false>\[")


def test_pass1_per_frame_raster(ipa, orc):
    spec = Spec("rgb8", "rgb8", 131, 113, 40)
    frames = Frames(spec, 3, util.SEED + 22100)
    check_route(ipa, orc, spec, frames, 3, OUT_U8, want_p1=0, tag_re=r"^ipk::k_raster_scale_down<unsigned char>$")


# ---------------------------------------------------------------------------------------------
# 4. scattered destinations, a chunk under 64, the fallbacks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [OUT_U8, OUT_F32])
def test_scattered_destinations(ipa, orc, out):
    """every second slot of a larger allocation: one chain launch per frame, the same results, the slots in between untouched"""
    L = ipa.lib()
    spec, frames = mosaic_frames("rggb", "u16")
    d = spec.desc(L, out)
    px3 = 23 * 17 * 3
    n = 5
    got, ran, names, _ = run_batch(ipa, d, frames.ptrs[:n], out, px3, slots=[2 * i for i in range(n)])
    assert len(batch_entries(ran)) == 1 and names == [S1] + [S2[out]] * n, (sorted(ran), names)
    packed, _, names_p, _ = run_batch(ipa, d, frames.ptrs[:n], out, px3)
    assert names_p == [S1, S2[out]]
    sentinel = np.array(util.SENTINELS[NP_OUT[out].name]).astype(NP_OUT[out])
    for i in range(n):
        same(got[2 * i], spec.oracle(orc, L, frames.host[i], out), "scattered frame %d" % i)
        same(got[2 * i], packed[i], "scattered frame %d against the packed batch" % i)
        if i:
            assert (got[2 * i - 1] == sentinel).all(), "the slot in front of frame %d was written" % i
    # two runs: frames 0..2 packed, a gap, frames 3..4 packed
    got, _, names, _ = run_batch(ipa, d, frames.ptrs[:n], out, px3, slots=[0, 1, 2, 4, 5])
    assert names == [S1, S2[out], S2[out]], names
    for i, s in enumerate([0, 1, 2, 4, 5]):
        same(got[s], packed[i], "two runs, frame %d" % i)
    assert (got[3] == sentinel).all()


def test_chunk_under_64(ipa, orc):
    """2048x1366 -> 1024x683: 23 frames per chunk, so 24 frames are a chunk of 23 and a chunk of one.  Pass 1 is the window-8 kernel per frame (skip 2)"""
    L = ipa.lib()
    spec = Spec("RGGB", "u16", 2048, 1366, 1024)
    assert br.sizes(L, spec.desc(L, OUT_U8))[:2] == (1024, 683) and br.chunk_of(1024, 683) == 23
    frames = Frames(spec, 24, util.SEED + 23000, derive=True)
    assert not np.array_equal(frames.host[0], frames.host[23])
    check_route(ipa, orc, spec, frames, 24, OUT_U8, want_p1=0, tag_re=r"^ipk::k_raw_scaled_demosaic_w8m<unsigned short, 3u, false>\[",
                oracle_frames=(0, 22, 23))


@pytest.mark.parametrize("what", ["n=1", "rotate90", "crop", "15x10"])
def test_fallbacks(ipa, orc, what):
    """not on the route: bit-identical to the loop, with the loop's stage labels"""
    L = ipa.lib()
    kw = dict(MOSAICS["rggb"])
    n = 3
    if what == "n=1":
        n = 1
    elif what == "rotate90":
        kw.update(rotation=1, maxheight=23)
    elif what == "crop":
        kw.update(rotatecrop=(0.1, 0.05, 0.08, 0.12, 0.0))
    else:
        kw.update(maxwidth=15)
    spec = Spec(src="u16", **kw)
    frames = Frames(spec, n, util.SEED + 24000 + len(what))
    out = OUT_U8
    d = spec.desc(L, out)
    dw, dh, fw, fh = br.sizes(L, d)
    if what == "15x10":
        assert dw == 15 and dw * dh < 256, (dw, dh)
    assert br.report(L, d, n, out) == (0, 0, 0)
    px3 = fw * fh * 3
    got, ran, names, used = run_batch(ipa, d, frames.ptrs, out, px3)
    singles, _, names1, used1 = run_singles(ipa, d, frames.ptrs, out, px3)
    assert not batch_entries(ran) and names == names1 * n and used == used1, (what, sorted(ran), names, names1)
    for i in range(n):
        same(got[i], singles[i], "%s: frame %d against ipk_pipeline_run" % (what, i))
        same(got[i], spec.oracle(orc, L, frames.host[i], out), "%s: frame %d against the oracle" % (what, i))


# ---------------------------------------------------------------------------------------------
# 5. the primitives
# ---------------------------------------------------------------------------------------------
def _rgbe_slices(ipa, n, px4, off, call):
    """a guarded n x px4 f32 destination, `off` floats past a 256-byte boundary"""
    import torch
    g = util.Guarded(n * px4, NP_OUT[OUT_F32], off=off)
    assert g.ptr % 16 == (4 * off) % 16
    with ipa.launch_log() as ran:
        assert call(g.ptr) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    return g.result("rgbe slices").reshape(n, px4), ran


@pytest.mark.parametrize("src", ["u16", "f32"])
def test_raw_primitive(ipa, src):
    """slice i is the single-frame call's result: the general-kernel geometry (aligned, and one float off a 16-byte boundary), and a window-8 geometry,
    which the same misalignment sends to the general kernel too"""
    import torch
    L = ipa.lib()
    spec, frames = mosaic_frames("rggb", src)
    x, y, w, h, ow = 5, 2, 203, 151, 211
    st = SRC_TYPE[src]
    n = 5
    sp = (C.c_void_p * n)(*frames.ptrs[:n])
    for nw, nh, off, general in ((23, 17, 0, True), (23, 17, 1, True), (60, 45, 0, False), (60, 45, 1, True)):
        px4 = nw * nh * 4
        args = (st, ow, x, y, w, h, util.BLACK, util.WHITE, b"RGGB", nw, nh)
        got, ran = _rgbe_slices(ipa, n, px4, off, lambda p: L.ipk_raw_scaled_demosaic_batch(sp, n, *args, p, None))
        if general:
            assert len(batch_entries(ran)) == 1 and len(ran) == 1 and re.match(mosaic_tag(src), batch_entries(ran)[0]), sorted(ran)
        else:
            assert not batch_entries(ran) and len(ran) == 1 and "k_raw_scaled_demosaic_w8m<" in list(ran)[0], sorted(ran)
        for i in range(n):
            one, ran1 = _rgbe_slices(ipa, 1, px4, off, lambda p: L.ipk_raw_scaled_demosaic(frames.ptrs[i], *args, p, None))
            assert not batch_entries(ran1) and ("_w8m<" in list(ran1)[0]) == (not general), sorted(ran1)
            util.assert_bits_equal(got[i], one[0], "%s %dx%d off %d: slice %d" % (src, nw, nh, off, i))
    # the Python wrapper
    got = ipa.raw_scaled_demosaic_batch(frames.views[:3], ow, x, y, w, h, util.BLACK, util.WHITE, "RGGB", 23, 17)
    one, _ = _rgbe_slices(ipa, 1, 23 * 17 * 4, 0, lambda p: L.ipk_raw_scaled_demosaic(frames.ptrs[2], st, ow, x, y, w, h, util.BLACK, util.WHITE, b"RGGB", 23, 17, p, None))
    torch.cuda.synchronize()
    util.assert_bits_equal(got.cpu().numpy().reshape(3, -1)[2], one[0], "the Python wrapper")


@pytest.mark.parametrize("kind,src", [("mono", "f32"), ("cpp3", "u16")])
def test_plain_primitive(ipa, kind, src):
    L = ipa.lib()
    spec = Spec(kind, src, 131, 113, 30)
    frames = Frames(spec, 4, util.SEED + 25000 + len(kind))
    fa = lambda v: (C.c_float * 4)(*[float(x) for x in v])
    b, wh = fa(B3), fa(W3)
    code = 2 if kind == "mono" else 1                                        # ipk_plain_kind
    n, nw, nh = 4, 13, 11
    args = (SRC_TYPE[src], code, 131, 5, 3, 120, 100, b, wh, nw, nh)
    sp = (C.c_void_p * n)(*frames.ptrs)
    for off in (0, 1):
        got, ran = _rgbe_slices(ipa, n, nw * nh * 4, off, lambda p: L.ipk_plain_scale_down_batch(sp, n, *args, p, None))
        assert len(ran) == 1 and re.search(r",plain=%d,batch=1\]$" % (1 if kind == "mono" else 3), list(ran)[0]), sorted(ran)
        for i in range(n):
            one, ran1 = _rgbe_slices(ipa, 1, nw * nh * 4, off, lambda p: L.ipk_plain_scale_down(frames.ptrs[i], *args, p, None))
            assert not batch_entries(ran1)
            util.assert_bits_equal(got[i], one[0], "%s %s off %d: slice %d" % (kind, src, off, i))
    got = ipa.plain_scale_down_batch(frames.views, code, 131, 5, 3, 120, 100, B3, W3, nw, nh)
    util.assert_bits_equal(got.cpu().numpy().reshape(n, -1)[3], one[0], "the Python wrapper")


def test_raster_kind_forwards_frame_by_frame(ipa):
    L = ipa.lib()
    spec = Spec("rgb8", "rgb8", 131, 113, 40)
    frames = Frames(spec, 3, util.SEED + 25500)
    args = (br.RGB8, 0, 131, 5, 3, 120, 100, None, None, 13, 11)
    sp = (C.c_void_p * 3)(*frames.ptrs)
    got, ran = _rgbe_slices(ipa, 3, 13 * 11 * 4, 0, lambda p: L.ipk_plain_scale_down_batch(sp, 3, *args, p, None))
    assert sorted(ran) == ["ipk::k_raster_scale_down<unsigned char>"], sorted(ran)
    for i in range(3):
        one, _ = _rgbe_slices(ipa, 1, 13 * 11 * 4, 0, lambda p: L.ipk_plain_scale_down(frames.ptrs[i], *args, p, None))
        util.assert_bits_equal(got[i], one[0], "raster slice %d" % i)


def test_primitives_empty_and_null(ipa):
    """n = 0: IPK_OK, nothing enqueued; a null frame pointer: IPK_ERR_INVALID, nothing enqueued"""
    import torch
    L = ipa.lib()
    spec, frames = mosaic_frames("rggb", "u16")
    out = torch.full((3 * 23 * 17 * 4,), 7.0, dtype=torch.float32, device="cuda")
    raw = (0, 211, 5, 2, 203, 151, util.BLACK, util.WHITE, b"RGGB", 23, 17)
    fa = (C.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    plain = (0, 2, 211, 5, 2, 203, 151, fa, fa, 23, 17)
    holed = (C.c_void_p * 3)(frames.ptrs[0], None, frames.ptrs[2])
    with ipa.launch_log() as ran:
        assert L.ipk_raw_scaled_demosaic_batch(None, 0, *raw, out.data_ptr(), None) == 0
        assert L.ipk_plain_scale_down_batch(None, 0, *plain, out.data_ptr(), None) == 0
        assert L.ipk_raw_scaled_demosaic_batch(holed, 3, *raw, out.data_ptr(), None) == -2
        assert L.ipk_plain_scale_down_batch(holed, 3, *plain, out.data_ptr(), None) == -2
        assert L.ipk_raw_scaled_demosaic_batch(None, 3, *raw, out.data_ptr(), None) == -2
        assert L.ipk_raw_scaled_demosaic_batch(holed, 1, *raw, None, None) == -2
        torch.cuda.synchronize()
    assert not ran, sorted(ran)
    assert bool((out == 7.0).all()), "a refused or empty call wrote to dst"


# ---------------------------------------------------------------------------------------------
# 6. the multi-device driver inherits the route
# ---------------------------------------------------------------------------------------------
def test_multi_device_driver_takes_the_route(ipa, orc):
    """ipk_pipeline_run_batch_multi where the current context takes every frame: no device set, or -- where an earlier module of the session left one
    -- a set of the one member on device 0, which deals every frame to that context as well"""
    L = ipa.lib()
    spec, frames = mosaic_frames("xtrans", "f32")
    had = L.ipk_device_set_size()
    if had > 0:
        ipa.init_devices([0])
    try:
        n, out = 6, OUT_U8
        d = spec.desc(L, out)
        fw, fh = br.sizes(L, d)[2:]
        got, ran, names, used = run_batch(ipa, d, frames.ptrs[:n], out, fw * fh * 3, multi=True)
        assert len(batch_entries(ran)) == 1 and re.match(mosaic_tag("f32"), batch_entries(ran)[0]), sorted(ran)
        assert names == [S1, S2[out]] and used == 0, names
        plain, _, _, _ = run_batch(ipa, d, frames.ptrs[:n], out, fw * fh * 3)
        for i in range(n):
            same(got[i], spec.oracle(orc, L, frames.host[i], out), "multi: frame %d against the oracle" % i)
            same(got[i], plain[i], "multi: frame %d against ipk_pipeline_run_batch" % i)
    finally:
        if had > 0:
            assert L.ipk_init_devices(None, 0) == 0
