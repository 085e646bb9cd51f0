"""The nine route switches crossed on the GPU: the cases and settings of tests/test_switch_matrix_route.py (ten sources x seven geometries; allow_fused
0..255 x fuse_rotatecrop x fuse_scaledown) through ipk_pipeline_run and ipk_pipeline_run_region, and one PipelineCache shared by two settings through
ipk_pipeline_run_cached and ipk_pipeline_run_cached_region.  The header's contract for every switch is "no result, no hash": so every setting must give
the CPU oracle's bits (f32 bit patterns, any NaN == any NaN; equal u8 / u16), and whatever a route stores under a cache key must be what the staged
driver stores there, because a follower under another setting reads it.  The comparisons run on the device; a result comes back only to report a
difference.  test_the_switches_change_what_is_launched asserts that the sweep is not vacuous."""
import ctypes as C

import numpy as np
import pytest

import util
import test_gpu_staged_paths as sp
import test_gpu_plain_route as pr
import test_gpu_buffer_bounds as bb
import test_switch_matrix_route as mr
from test_switch_matrix_route import W, H, ON, ALL_ON, SWITCHES, SOURCES, GEOMETRIES, CASES, CASE_IDS, S260, N_SETTINGS, setting

pytestmark = pytest.mark.gpu

OUT = [sp.F32, sp.U8, sp.U16]
NP_OUT = [np.dtype(np.float32), np.dtype(np.uint8), np.dtype(np.uint16)]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
_DATA, _BUILT = {}, {}


def _data(name):
    """the source's samples, one frame per source; f32 frames hold util.SPECIALS scaled to the white level and lone non-finite samples, each alone in an
    ordinary neighbourhood (test_gpu_plain_previews._frame's placement)"""
    if name not in _DATA:
        seed = util.SEED + 19000 + 16 * SOURCES.index(name)
        if name in mr.RASTERS:
            _DATA[name] = (pr._image(name, H, W, seed), None)
        else:
            data, src = sp._source(name, H, W, seed)
            if src["is_float"]:
                spp = src["cpp"]
                flat = data.reshape(H, W * spp)
                with np.errstate(over="ignore"):
                    spc = util.SPECIALS * np.float32(src["whitelevels"][0])
                for k in range(0, spc.size, W * spp):
                    part = spc[k: k + W * spp]
                    flat[1 + 2 * (k // (W * spp)), :part.size] = part
                flat[H // 2, (W // 2) * spp] = -np.inf
                flat[H - 2, 3 * spp + spp - 1] = np.nan
                flat[5, (W - 2) * spp] = np.inf
            _DATA[name] = (data, src)
    return _DATA[name]


def _make(ipa, orc, i, j, **edit):
    """(pipeline, a maker of fresh oracle descriptors) of case (i, j); edit: ops laid over the case's (exposure, linear)"""
    import torch
    name = SOURCES[i]
    data, src = _data(name)
    crops, ops = mr.case_ops(orc, i, j)
    if name in mr.RASTERS:
        ops = dict(ops, exposure=mr.RASTER_EXPOSURE)
    ops.update(edit)
    if name in mr.RASTERS:                                                # test_gpu_plain_route._build's raster arm
        dev = torch.from_numpy(data.ravel()).cuda() if name == "rgb8" else ipa.upload_u16(data)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(W, H, dev, bits=8 if name == "rgb8" else 16))
        g = pipe.ops.gofloat
        g.crop_top, g.crop_right, g.crop_bottom, g.crop_left = crops
        sp._apply(pipe, ops)
        return pipe, (lambda **kw: orc.make_pipeline(data, crops=crops, **dict(ops, **kw)))
    pipe = sp._pipeline(ipa, data, src, crops, ops)
    return pipe, (lambda **kw: sp._oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=util.WB, cam_to_xyz_normalized=sp._cam4(), **kw)))


def _case(ipa, orc, i, j):
    """the case's pipeline, its output type and the oracle's result of that type: computed once, shared, never written"""
    if (i, j) not in _BUILT:
        pipe, desc = _make(ipa, orc, i, j)
        t = mr.out_type_of(i, j)
        want = sp._want(orc, desc(), OUT[t])
        _, (fw, fh) = pipe.sizes()
        assert want.shape == (fh, fw, 3) and want.dtype == NP_OUT[t], CASE_IDS[CASES.index((i, j))]
        want.setflags(write=False)
        _BUILT[(i, j)] = (pipe, t, want, mr.regions_of(fw, fh))
    return _BUILT[(i, j)]


# ---------------------------------------------------------------------------------------------
# the four drivers behind one call, and the comparison on the device
# ---------------------------------------------------------------------------------------------
def _drive(ipa, d, src, out_type, dst_ptr, region=None, cache=None):
    """ipk_pipeline_run / _run_region / _run_cached / _run_cached_region by what is given -> (status, used_fused or windowed, ops_run)"""
    L = ipa.lib()
    flag, mask = C.c_int(-1), C.c_int(-1)
    sptr, dptr = C.c_void_p(src.data_ptr()), C.c_void_p(dst_ptr)
    if cache is None and region is None:
        rc = L.ipk_pipeline_run(C.byref(d), sptr, dptr, out_type, C.byref(flag), ipa._stream())
    elif cache is None:
        rc = L.ipk_pipeline_run_region(C.byref(d), sptr, *region, dptr, out_type, C.byref(flag), ipa._stream())
    elif region is None:
        rc = L.ipk_pipeline_run_cached(C.byref(d), sptr, 0, cache.handle, out_type, dptr, C.byref(mask), C.byref(flag), ipa._stream())
    else:
        rc = L.ipk_pipeline_run_cached_region(C.byref(d), sptr, 0, cache.handle, *region, dptr, out_type, C.byref(mask), C.byref(flag), ipa._stream())
    return rc, flag.value, mask.value


def _to_device(a):
    import torch
    a = np.array(a, copy=True).ravel()                                       # the shared oracle results are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _differ(got, want):
    """on the device: integer views, any NaN == any NaN"""
    import torch
    if got.dtype == torch.float32:
        ne = (got.view(torch.int32) != want.view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
    else:
        ne = got != want
    return bool(ne.any())


def _first_difference(got, want_host, out_type):
    a = got.cpu().numpy()
    a = a.view(np.uint16) if out_type == 2 else a
    try:
        sp._same(a.reshape(want_host.shape), want_host, "")
    except AssertionError as e:
        return str(e).lstrip(": ")
    return "the device comparison and the host comparison disagree"


def _sentinel(t):
    return util.SENTINELS[util._np_dtype(t.dtype).name]


def _name(s):
    return "allow_fused=%d fuse_rotatecrop=%d fuse_scaledown=%d" % setting(s)


def _region_of(want, reg):
    x, y, w, h = reg
    return np.ascontiguousarray(want[y:y + h, x:x + w])


# ---------------------------------------------------------------------------------------------
# a. whole frames under all 1024 settings, regions under S260, uncached
# ---------------------------------------------------------------------------------------------
SWEEP = list(range(N_SETTINGS))
# the settings whose launches are recorded for test_the_switches_change_what_is_launched: each switch alone beside bit 0 and each switch alone missing
LOGGED = sorted({0, ON, ALL_ON} | {ON | b for b in SWITCHES.values()} | {ALL_ON ^ b for b in SWITCHES.values()})
_LOGS = {}


def _sweep_case(ipa, orc, i, j, f, whole_settings, region_settings):
    """every setting against the oracle; findings go to f.errs, the launch logs of LOGGED to _LOGS[(i, j)]"""
    import torch
    torch_dt = {0: torch.float32, 1: torch.uint8, 2: torch.int16}
    pipe, t, want, regs = _case(ipa, orc, i, j)
    L = ipa.lib()
    src = pipe.globals.image.data
    d = pipe.desc()
    want_dev = _to_device(want)
    reg_host = [_region_of(want, r) for r in regs]
    reg_dev = [_to_device(r) for r in reg_host]
    out = torch.empty(want.size, dtype=torch_dt[t], device="cuda")
    reg_out = [torch.empty(r.size, dtype=torch_dt[t], device="cuda") for r in reg_host]
    logs = _LOGS.setdefault((i, j), {})

    def whole(s):
        mr.apply_setting(d, s)
        out.fill_(_sentinel(out))
        rc, _, _ = _drive(ipa, d, src, t, out.data_ptr())
        if rc != 0:
            f.errs.append("[status] %s: ipk_pipeline_run %d (%s)" % (_name(s), rc, L.ipk_last_error().decode()))
        elif _differ(out, want_dev):
            f.errs.append("[parity] %s, whole frame: %s" % (_name(s), _first_difference(out, want, t)))

    def regions(s):
        mr.apply_setting(d, s)
        for k, reg in enumerate(regs):
            plan = L.ipk_pipeline_region(C.byref(d), t, *reg, *[C.byref(C.c_size_t()) for _ in range(4)])
            what = "%s, region %r" % (_name(s), reg)
            if s in (ALL_ON, ON):                                            # guard bands, one element past a 256-byte boundary
                g = util.Guarded(reg_host[k].size, NP_OUT[t], 1)
                rc, windowed, _ = _drive(ipa, d, src, t, g.ptr, region=reg)
                if rc == 0:
                    f.verify(g, reg_host[k], what)
            else:
                o = reg_out[k]
                o.fill_(_sentinel(o))
                rc, windowed, _ = _drive(ipa, d, src, t, o.data_ptr(), region=reg)
                if rc == 0 and _differ(o, reg_dev[k]):
                    f.errs.append("[parity] %s: %s" % (what, _first_difference(o, reg_host[k], t)))
            if rc != 0:
                f.errs.append("[status] %s: ipk_pipeline_run_region %d (%s)" % (what, rc, L.ipk_last_error().decode()))
            elif windowed != plan:
                f.errs.append("[plan] %s: ipk_pipeline_run_region says windowed = %d, ipk_pipeline_region returns %d" % (what, windowed, plan))

    def cold_cached_region(s):
        """IPK_FUSED_CACHED_RESAMPLE concerns ipk_pipeline_run_cached_region alone: one region from an empty cache joins the recorded launches"""
        mr.apply_setting(d, s)
        cache = ipa.PipelineCache(1 << 26)
        try:
            o = reg_out[1]
            o.fill_(_sentinel(o))
            rc, _, _ = _drive(ipa, d, src, t, o.data_ptr(), region=regs[1], cache=cache)
            if rc != 0:
                f.errs.append("[status] %s: ipk_pipeline_run_cached_region %d (%s)" % (_name(s), rc, L.ipk_last_error().decode()))
            elif _differ(o, reg_dev[1]):
                f.errs.append("[parity] %s, region %r from an empty cache: %s" % (_name(s), regs[1], _first_difference(o, reg_host[1], t)))
            torch.cuda.synchronize()
        finally:
            cache.close()

    region_settings = set(region_settings)
    for s in whole_settings:
        if s in LOGGED:
            with ipa.launch_log() as ran_whole:
                whole(s)
                torch.cuda.synchronize()
            with ipa.launch_log() as ran_rest:
                regions(s)
                cold_cached_region(s)
                torch.cuda.synchronize()
            logs[s] = (frozenset(ran_whole), frozenset(ran_whole | ran_rest))
        else:
            whole(s)
            if s in region_settings:
                regions(s)
    torch.cuda.synchronize()


def _report(f):
    assert not f.errs, "%s: %d findings; the first of them:\n%s" % (f.cid, len(f.errs), "\n".join(f.errs[:12]))


@pytest.mark.parametrize("i,j", CASES, ids=CASE_IDS)
def test_every_setting_gives_the_oracles_bits(ipa, orc, i, j):
    """all 1024 settings through ipk_pipeline_run, S260 through ipk_pipeline_run_region (two regions)"""
    assert set(LOGGED) <= set(S260) | {0}
    f = bb.Findings(CASE_IDS[CASES.index((i, j))])
    _sweep_case(ipa, orc, i, j, f, SWEEP, S260)
    _report(f)


# ---------------------------------------------------------------------------------------------
# c. the sweep exercises something
# ---------------------------------------------------------------------------------------------
def test_the_switches_change_what_is_launched(ipa, orc):
    """every switch changes the set of launched kernels on some case (whole frame, the two regions and one region from an empty cache, beside bit 0
    alone or taken out of the all-on setting), and all-on launches fewer DISTINCT kernels for the whole frame than (0, 0, 0) on some case of every
    source.  launch_log() yields the set of kernel names, not a count of launches: a route that launches one kernel twice counts once."""
    for i, j in CASES:                                                       # cases the sweep above has not run in this session: the logged settings alone
        if len(_LOGS.get((i, j), {})) < len(LOGGED):
            f = bb.Findings(CASE_IDS[CASES.index((i, j))])
            _sweep_case(ipa, orc, i, j, f, LOGGED, ())
            _report(f)
    for name, bit in SWITCHES.items():
        moved = [CASE_IDS[CASES.index(c)] for c in CASES
                 if _LOGS[c][ON][1] != _LOGS[c][ON | bit][1] or _LOGS[c][ALL_ON][1] != _LOGS[c][ALL_ON ^ bit][1]]
        assert moved, "%s changes the launched kernels on no case" % name
        beside_all = [CASE_IDS[CASES.index(c)] for c in CASES if _LOGS[c][ALL_ON][1] != _LOGS[c][ALL_ON ^ bit][1]]
        assert beside_all, "%s changes the launched kernels on no case once every other switch is set" % name
    for i, name in enumerate(SOURCES):
        fewer = [GEOMETRIES[j][0] for j in range(len(GEOMETRIES)) if len(_LOGS[(i, j)][ALL_ON][0]) < len(_LOGS[(i, j)][0][0])]
        assert fewer, "%s: all-on launches no fewer distinct kernels than (0, 0, 0) on any geometry: %r" % (
            name, {GEOMETRIES[j][0]: (sorted(_LOGS[(i, j)][0][0]), sorted(_LOGS[(i, j)][ALL_ON][0])) for j in range(len(GEOMETRIES))})


# ---------------------------------------------------------------------------------------------
# b. one cache, two settings
# ---------------------------------------------------------------------------------------------
T_SETTINGS = [0, ON] + [ON | b for b in SWITCHES.values()] + [ALL_ON]
PAIRS = [(ia, ib) for ia in range(len(T_SETTINGS)) for ib in range(len(T_SETTINGS))]
CACHE_SOURCES = ["bayer", "xtrans", "rgbe", "mono_u16", "rgb3_f32", "rgb8"]
CACHE_CASES = [(SOURCES.index(n), j) for n in CACHE_SOURCES for j in (1, 6)]
EDIT = 0.5


def _entry(ipa, cache, key):
    """(width, height, channels, mono, bits as uint32) of a memoised buffer, or None"""
    L = ipa.lib()
    p, w, h, c, m = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    rc = L.ipk_cache_get(cache.handle, key, C.byref(p), C.byref(w), C.byref(h), C.byref(c), C.byref(m))
    if rc != 0:
        assert rc == 1, rc
        return None
    bits = np.empty(w.value * h.value * c.value, np.uint32)
    assert L.ipk_stream_sync(ipa._stream()) == 0
    assert L.ipk_memcpy_d2h(bits.ctypes.data, p, bits.nbytes, None) == 0
    return (w.value, h.value, c.value, m.value), bits


def _bits_differ(a, b):
    if a.shape != b.shape:
        return True
    ne = a != b
    if not ne.any():
        return False
    return bool((ne & ~(np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32)))).any())


def _stage_buffer(orc, name, data, src, crops, dw, dh):
    """the oracle's OpGoFloat + OpDemosaic result: what the cache must hold under the demosaic hash (tests/test_cache_contract.py)"""
    x, y, cw, ch = orc.size_image(*crops, W, H)
    with np.errstate(all="ignore"):
        if name in mr.RASTERS:
            buf, cfa = orc.gofloat_other(data, x, y, cw, ch), ""
        elif src["cfa"]:
            buf, cfa = orc.gofloat_cfa(data, x, y, cw, ch, src["blacklevels"][0], src["whitelevels"][0]), orc.cfa_shift(src["cfa"], crops[3], crops[0])
        elif src["cpp"] == 3:
            buf, cfa = orc.gofloat_rgb(data, x, y, cw, ch, src["blacklevels"], src["whitelevels"]), ""
        else:
            buf, cfa = orc.gofloat_mono(data, x, y, cw, ch, src["blacklevels"][0], src["whitelevels"][0]), ""
        return orc.demosaic_run(cfa, buf, dw, dh)[1]


_SNAPSHOTS = {}


def _snapshot(ipa, orc, i, j):
    """what a cache filled by (0, 0, 0) alone holds, at the case's exposure and at the edited one: {key: entry}; the demosaic and final buffers are the
    oracle's.  Also the oracle's results and the keys per exposure.  Once per case."""
    import torch
    if (i, j) in _SNAPSHOTS:
        return _SNAPSHOTS[(i, j)]
    pipe, t, want, regs = _case(ipa, orc, i, j)
    _, desc = _make(ipa, orc, i, j)
    name = SOURCES[i]
    data, src = _data(name)
    crops, _ = mr.case_ops(orc, i, j)
    wants = {None: want, EDIT: sp._want(orc, desc(exposure=EDIT), OUT[t])}
    snap, keys = {}, {}
    cache = ipa.PipelineCache(1 << 28)
    out = torch.empty(want.size, dtype={0: torch.float32, 1: torch.uint8, 2: torch.int16}[t], device="cuda")
    base = pipe.ops.basecurve.exposure
    try:
        for e in (None, EDIT):
            pipe.ops.basecurve.exposure = base if e is None else e
            d = mr.apply_setting(pipe.desc(), 0)
            keys[e] = pipe.hashes(t)
            rc, _, mask = _drive(ipa, d, pipe.globals.image.data, t, out.data_ptr(), cache=cache)
            assert rc == 0 and not _differ(out, _to_device(wants[e])), (CASE_IDS[CASES.index((i, j))], e, rc)
            for k, key in enumerate(keys[e]):
                got = _entry(ipa, cache, key)
                if got is not None:
                    snap[key] = got
            # the final buffer is the oracle's f32 result under the `linear` the output type forces; the demosaic buffer its gofloat + demosaic
            final = orc.pipeline_run(desc(linear=t == 2, **({} if e is None else dict(exposure=e))))
            meta, bits = snap[keys[e][7]]
            assert meta[:3] == (final.shape[1], final.shape[0], 3) and not _bits_differ(bits, final.ravel().view(np.uint32)), "memoised final buffer"
            if e is None:                                                    # hashes 0..3 do not see the exposure
                assert keys[e][1] in snap, "the staged driver did not memoise the demosaic buffer: nothing to compare the other settings with"
                (dw, dh), _ = pipe.sizes()
                dem = _stage_buffer(orc, name, data, src, crops, dw, dh)
                meta, bits = snap[keys[e][1]]
                assert meta == (dem.shape[1], dem.shape[0], 4, int(name.startswith("mono"))), (meta, dem.shape)
                assert not _bits_differ(bits, np.ascontiguousarray(dem).ravel().view(np.uint32)), "memoised demosaic buffer"
    finally:
        pipe.ops.basecurve.exposure = base
        cache.close()
    assert keys[None][:4] == keys[EDIT][:4] and all(a != b for a, b in zip(keys[None][4:], keys[EDIT][4:]))
    # the oracle's results on the device, once: dev[exposure, None] the whole frame, dev[exposure, k] region k
    dev = {(e, k): _to_device(wants[e] if k is None else _region_of(wants[e], regs[k])) for e in wants for k in (None, 0, 1)}
    _SNAPSHOTS[(i, j)] = (snap, keys, wants, dev)
    return _SNAPSHOTS[(i, j)]


def _pair(ipa, orc, i, j, ia, ib, f):
    """settings A = T_SETTINGS[ia] and B = T_SETTINGS[ib] on one cache, three times from a fresh one; after each step the cache against the (0, 0, 0)
    snapshot.
      1. a region under A, then the whole frame under B: with IPK_FUSED_CACHED_RESAMPLE in A the follower's whole run meets a cache without the
         rotatecrop buffer; then a region under B, then the exposure edit under B (region, whole frame).
      2. the whole frame under A, then a region and the whole frame under B, then the edit.
      3. regions alone, A's and straight after it B's: B's region route meets the cache as A's region left it.
    Every pair runs all three.  Sequence 1 uses region (ia + ib) % 2, sequence 2 the other one, sequence 3 the first again: every B meets both
    regions, the one below 256 pixels included."""
    import torch
    a, b = T_SETTINGS[ia], T_SETTINGS[ib]
    pipe, t, want, regs = _case(ipa, orc, i, j)
    snap, keys, wants, dev = _snapshot(ipa, orc, i, j)
    L = ipa.lib()
    src = pipe.globals.image.data
    dt = {0: torch.float32, 1: torch.uint8, 2: torch.int16}[t]
    out = torch.empty(want.size, dtype=dt, device="cuda")
    reg_out = [torch.empty(r[2] * r[3] * 3, dtype=dt, device="cuda") for r in regs]
    base = pipe.ops.basecurve.exposure
    tag = "A = (%s), B = (%s)" % (_name(a), _name(b))
    caches = []

    def step(s, e, k, what):
        """k: the region's index, None for the whole frame"""
        cache = caches[-1]
        pipe.ops.basecurve.exposure = base if e is None else e
        d = mr.apply_setting(pipe.desc(), s)
        o = out if k is None else reg_out[k]
        o.fill_(_sentinel(o))
        rc, _, mask = _drive(ipa, d, src, t, o.data_ptr(), region=None if k is None else regs[k], cache=cache)
        what = "%s; %s%s" % (tag, what, "" if k is None else " (region %r)" % (regs[k],))
        if rc != 0:
            f.errs.append("[status] %s: %d (%s)" % (what, rc, L.ipk_last_error().decode()))
            return ()
        filled = []
        if _differ(o, dev[e, k]):
            w = wants[e] if k is None else _region_of(wants[e], regs[k])
            f.errs.append("[parity] %s (ops_run 0x%02x): %s" % (what, mask, _first_difference(o, w, t)))
        for n, key in enumerate(keys[e]):
            got = _entry(ipa, cache, key)
            if got is None:
                continue                                                     # a key a setting does not fill is fine
            filled.append(n)
            if key not in snap:
                f.errs.append("[cache] %s: hash %d is filled, which (0, 0, 0) never fills: nothing vouches for it" % (what, n))
            elif got[0] != snap[key][0]:
                f.errs.append("[cache] %s: hash %d holds (w, h, channels, mono) = %r, the staged driver stores %r" % (what, n, got[0], snap[key][0]))
            elif _bits_differ(got[1], snap[key][1]):
                ne = np.flatnonzero(got[1] != snap[key][1])
                f.errs.append("[cache] %s: hash %d holds other bits than the staged driver stores: %d samples, first at %d (channel %d): 0x%08x, staged 0x%08x" % (
                    what, n, ne.size, ne[0], ne[0] % got[0][2], got[1][ne[0]], snap[key][1][ne[0]]))
        return filled

    def edit(k):
        step(b, EDIT, k, "then a region under B with the exposure at %g" % EDIT)
        step(b, EDIT, None, "then the whole frame under B with the exposure at %g" % EDIT)

    k1 = (ia + ib) % 2
    k2 = 1 - k1
    both = mr.apply_setting(pipe.desc(), a & b)
    resamples = bool(a & b & mr.CACHED) and L.ipk_pipeline_resamples_cached_region(C.byref(both), t) == 1
    try:
        caches.append(ipa.PipelineCache(1 << 28))
        filled = step(a, None, k1, "a region under A")
        if a & mr.CACHED and a & ON and 2 in filled and L.ipk_pipeline_resamples_cached_region(C.byref(mr.apply_setting(pipe.desc(), a)), t) == 1:
            f.errs.append("[cache] %s: A's region filled the rotatecrop hash under IPK_FUSED_CACHED_RESAMPLE: the follower does not meet the cache this sequence is about" % tag)
        step(b, None, None, "a region under A, then the whole frame under B")
        step(b, None, k1, "a region under A, the whole frame under B, then a region under B")
        edit(k1)
        caches.append(ipa.PipelineCache(1 << 28))
        step(a, None, None, "the whole frame under A")
        step(b, None, k2, "the whole frame under A, then a region under B")
        step(b, None, None, "the whole frame under A, a region under B, then the whole frame under B")
        edit(k2)
        caches.append(ipa.PipelineCache(1 << 28))
        step(a, None, k1, "regions alone: a region under A")
        filled = step(b, None, k1, "regions alone: a region under A, then a region under B")
        if resamples and 2 in filled:
            f.errs.append("[cache] %s: two regions under IPK_FUSED_CACHED_RESAMPLE filled the rotatecrop hash: the resampling route was not the one taken" % tag)
        step(b, EDIT, k1, "regions alone: a region under A, then under B, then under B with the exposure at %g" % EDIT)
        torch.cuda.synchronize()
    finally:
        pipe.ops.basecurve.exposure = base
        for cache in caches:
            cache.close()


@pytest.mark.parametrize("i,j", CACHE_CASES, ids=[CASE_IDS[CASES.index(c)] for c in CACHE_CASES])
def test_one_cache_two_settings(ipa, orc, i, j):
    """every ordered pair (A, B) of T_SETTINGS, A == B included, in both step orders and with regions alone (_pair)"""
    f = bb.Findings(CASE_IDS[CASES.index((i, j))])
    for ia, ib in PAIRS:
        _pair(ipa, orc, i, j, ia, ib, f)
    _report(f)
