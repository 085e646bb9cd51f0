"""Edit sessions on caches too small to hold them, on the GPU: the sessions of tests/test_cache_pressure_model.py (a fixed script of edits and a seeded
random tail, thirteen descriptors, seven budgets from 0 to 1 << 28) replayed through ipk_pipeline_run_cached and ipk_pipeline_run_cached_region on a real
PipelineCache of each budget.  After every step: the pixels against the CPU oracle for the descriptor then in force (compared on the device; f32 bit
patterns, any NaN == any NaN), ops_run / windowed / used_fused against the model, the key set, bytes, entries and evictions against the model, and every
memoised buffer against the shape the model derives for its key and the bits a switches-off run on an unlimited cache stores under it (whose demosaic
and final buffers are the oracle's).  At three budgets the session runs once more with nothing between the calls -- no read, no synchronisation, a
destination per step -- which is the header's claim that a buffer evicted by the next call outlives the launch that reads it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_staged_paths as sp
import test_gpu_buffer_bounds as bb
import test_switch_matrix_route as mr
import test_gpu_switch_matrix as gm
import test_cache_pressure_model as pm
from test_switch_matrix_route import SOURCES

pytestmark = pytest.mark.gpu

NP_OUT = gm.NP_OUT
ORACLE_OUT = [sp.F32, sp.U8, sp.U16]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


# ---------------------------------------------------------------------------------------------
# a case: two frames on the device, the oracle's results and the reference cache contents, memoised over the budgets
# ---------------------------------------------------------------------------------------------
class Case:
    def __init__(self, ipa, orc, case):
        import torch
        self.case, self.cid = case, pm.SESSION_IDS[pm.SESSION_CASES.index(case)]
        self.name = "rgb8" if case == pm.FASTPATH else SOURCES[case[0]]
        self.session = pm.session(ipa.lib(), orc, case)
        self.frames = pm.frames_of(case)                                       # (samples, RawImage fields or None)
        self.dev = []
        for data, src in self.frames:
            if src is None:
                self.dev.append(torch.from_numpy(data.ravel()).cuda() if data.dtype == np.uint8 else ipa.upload_u16(data))
            else:
                self.dev.append(sp._upload(ipa, data, src["is_float"]))
        self.wants, self.wants_dev, self.snap = {}, {}, {}

    def oracle_desc(self, orc, d, frame, **kw):
        return pm.oracle_desc(orc, self.frames[frame][0], d, **kw)

    def want(self, orc, st, region=None):
        """the oracle's result of a state (or a rectangle of it) on the device, and on the host: once per descriptor, never written"""
        key = pm.Session.state_key(dict(st, setting=0))
        if key not in self.wants:
            d, out_type, _ = self.session.descs[pm.Session.state_key(st)]
            w = sp._want(orc, self.oracle_desc(orc, d, st["frame"]), ORACLE_OUT[out_type])
            r = self.session.reports[pm.Session.state_key(st)]
            assert w.shape == (r.fh, r.fw, 3) and w.dtype == NP_OUT[out_type], (self.cid, st, w.shape, w.dtype)
            w.setflags(write=False)
            self.wants[key] = w
        if (key, region) not in self.wants_dev:
            w = self.wants[key]
            self.wants_dev[key, region] = gm._to_device(w if region is None else gm._region_of(w, region))
        w = self.wants[key]
        return self.wants_dev[key, region], (w if region is None else gm._region_of(w, region))

    def reference(self, ipa, orc, st):
        """what a switches-off whole-frame run on an unlimited cache stores under the keys of a state: into self.snap, once per chain.  Its demosaic
        buffer is the oracle's gofloat + demosaic, its final buffer the oracle's f32 result under the `linear` the output type forces"""
        import torch
        k = pm.Session.state_key(st)
        r = self.session.reports[k]
        if r.fastpath or r.keys[7] in self.snap:
            return
        d, out_type, sid = self.session.descs[k]
        d = mr.apply_setting(pm.copy_desc(d), 0)
        cache = ipa.PipelineCache(1 << 28)
        try:
            out = torch.empty(r.fw * r.fh * 3, dtype=TORCH_OUT()[out_type], device="cuda")
            rc, _, mask = _drive(ipa, d, self.dev[st["frame"]], sid, out_type, out.data_ptr(), cache)
            assert rc == 0 and mask == 0xFF, (self.cid, st, rc, mask, ipa.lib().ipk_last_error())
            for n, key in enumerate(r.keys):
                got = gm._entry(ipa, cache, key)
                if got is not None:
                    self.snap[key] = got
        finally:
            cache.close()
        data, src = self.frames[st["frame"]]
        final = orc.pipeline_run(self.oracle_desc(orc, d, st["frame"], linear={0: bool(d.linear), 1: False, 2: True}[out_type]))
        meta, bits = self.snap[r.keys[7]]
        assert meta[:3] == (final.shape[1], final.shape[0], 3) and not gm._bits_differ(bits, final.ravel().view(np.uint32)), (self.cid, st, "final buffer")
        crops = (d.crop_top, d.crop_right, d.crop_bottom, d.crop_left)
        dem = gm._stage_buffer(orc, self.name, data, src, crops, r.dw, r.dh)
        meta, bits = self.snap[r.keys[1]]
        assert meta == (dem.shape[1], dem.shape[0], 4, int(self.name.startswith("mono"))), (self.cid, st, meta, dem.shape)
        assert not gm._bits_differ(bits, np.ascontiguousarray(dem).ravel().view(np.uint32)), (self.cid, st, "demosaic buffer")


_TORCH_OUT = []


def TORCH_OUT():
    import torch
    if not _TORCH_OUT:
        _TORCH_OUT.extend([torch.float32, torch.uint8, torch.int16])
    return _TORCH_OUT


_CASES = {}


def _case(ipa, orc, case):
    if case not in _CASES:
        _CASES[case] = Case(ipa, orc, case)
    return _CASES[case]


def _drive(ipa, d, src, source_id, out_type, dst_ptr, cache, region=None):
    """-> (status, used_fused or windowed, ops_run)"""
    L = ipa.lib()
    flag, mask = C.c_int(-1), C.c_int(-1)
    sptr, dptr = C.c_void_p(src.data_ptr()), C.c_void_p(dst_ptr)
    if region is None:
        rc = L.ipk_pipeline_run_cached(C.byref(d), sptr, source_id, cache.handle, out_type, dptr, C.byref(mask), C.byref(flag), ipa._stream())
    else:
        rc = L.ipk_pipeline_run_cached_region(C.byref(d), sptr, source_id, cache.handle, *region, dptr, out_type, C.byref(mask), C.byref(flag),
                                              ipa._stream())
    return rc, flag.value, mask.value


def _stats(ipa, cache):
    st = cache.stats()
    return st["bytes"], st["entries"], st["hits"], st["misses"], st["evictions"]


def _describe(n, st, action, region):
    edits = ", ".join("%s=%s" % (k, v) for k, v in sorted(st.items()) if v != pm.START.get(k) or k in ("out", "setting"))
    return "step %d (%s%s; %s)" % (n, action, "" if region is None else " %r" % (region,), edits)


# ---------------------------------------------------------------------------------------------
# the observed replay
# ---------------------------------------------------------------------------------------------
def _replay_observed(ipa, orc, c, budget, f):
    import torch
    L = ipa.lib()
    s = c.session
    m = pm.SessionModel(budget)
    cache = ipa.PipelineCache(budget)
    tag = "budget %d" % budget
    try:
        for n, (st, action) in enumerate(s.steps):
            k = pm.Session.state_key(st)
            r = s.reports[k]
            region = None if action in ("whole", "clear", "borrow") else s.regions(st)[action]
            what = "%s, %s" % (tag, _describe(n, st, action, region))
            if action == "clear":
                cache.clear()
                m.clear()
            elif action == "borrow":
                got = L.ipk_cache_get(cache.handle, r.keys[0], None, None, None, None, None)
                if got != (0 if m.cache.get(r.keys[0]) else 1):
                    f.errs.append("[keys] %s: ipk_cache_get of hash 0 returns %d" % (what, got))
            else:
                c.reference(ipa, orc, st)
                d, out_type, sid = s.descs[k]
                want_dev, want = c.want(orc, st, region)
                rec = m.call(r, region)
                o = torch.empty(want.size, dtype=TORCH_OUT()[out_type], device="cuda")
                o.fill_(gm._sentinel(o))
                rc, flag, mask = _drive(ipa, d, c.dev[st["frame"]], sid, out_type, o.data_ptr(), cache, region)
                if rc != 0:
                    f.errs.append("[status] %s: %d (%s)" % (what, rc, L.ipk_last_error().decode()))
                else:
                    if gm._differ(o, want_dev):
                        f.errs.append("[parity] %s, %s p=%s: %s" % (what, rec["form"], rec["p"], gm._first_difference(o, want, out_type)))
                    model_flag = rec["used_fused"] if region is None else rec["windowed"]
                    if (mask, flag) != (rec["ops_run"], model_flag):
                        f.errs.append("[report] %s: ops_run 0x%02x and %s %d; the model (%s, p=%s): 0x%02x and %d" % (
                            what, mask, "used_fused" if region is None else "windowed", flag, rec["form"], rec["p"], rec["ops_run"], model_flag))
            # the contents of the cache: every key the session has produced, in ascending order; a read refreshes recency, in the model too
            for key in sorted(m.shapes):
                present = m.cache.get(key)
                got = gm._entry(ipa, cache, key)
                if (got is not None) != present:
                    f.errs.append("[keys] %s: a key stored as hash %s is %s, in the model %s" % (
                        what, _which(s, key), "present" if got is not None else "absent", "present" if present else "absent"))
                if got is None:
                    continue
                if got[0] != m.shapes[key]:
                    f.errs.append("[shape] %s: hash %s holds (w, h, channels, mono) = %r, the model derives %r" % (what, _which(s, key), got[0], m.shapes[key]))
                if key not in c.snap:
                    f.errs.append("[contents] %s: hash %s is filled, which the switches-off run never fills" % (what, _which(s, key)))
                elif got[0] != c.snap[key][0] or not (np.array_equal(got[1], c.snap[key][1]) or not gm._bits_differ(got[1], c.snap[key][1])):
                    f.errs.append("[contents] %s: hash %s holds %r, not the %r the switches-off run stores, or other bits" % (
                        what, _which(s, key), got[0], c.snap[key][0]))
            b, e, _, _, ev = _stats(ipa, cache)
            if (b, e, ev) != (m.cache.bytes, len(m.cache.order), m.cache.evictions):
                f.errs.append("[stats] %s: bytes, entries, evictions = %r, the model %r" % (what, (b, e, ev), (m.cache.bytes, len(m.cache.order), m.cache.evictions)))
            if b > budget and e > 1:
                f.errs.append("[stats] %s: %d bytes in %d entries under a budget of %d" % (what, b, e, budget))
            if len(f.errs) > 40:
                f.errs.append("... stopped after step %d" % n)
                break
        torch.cuda.synchronize()
    finally:
        cache.close()


def _which(s, key):
    for k, r in s.reports.items():
        if key in r.keys:
            return "%d" % r.keys.index(key)
    return "?"


# ---------------------------------------------------------------------------------------------
# the unobserved replay: documented behaviour, run once
# ---------------------------------------------------------------------------------------------
def _replay_unobserved(ipa, orc, c, budget, f):
    """nothing between the calls: no ipk_cache_get but the session's own "borrow" steps, no host read, no synchronisation but the one inside the
    session's own ipk_cache_clear steps; every step writes to a destination of its own; one synchronisation at the end"""
    import torch
    L = ipa.lib()
    s = c.session
    m = pm.SessionModel(budget)
    tag = "budget %d, unobserved" % budget
    plan = []
    for n, (st, action) in enumerate(s.steps):                                 # everything the comparison needs, before the first call
        if action in ("clear", "borrow"):
            plan.append(None)
            continue
        region = None if action == "whole" else s.regions(st)[action]
        want_dev, want = c.want(orc, st, region)
        out_type = s.descs[pm.Session.state_key(st)][1]
        o = torch.empty(want.size, dtype=TORCH_OUT()[out_type], device="cuda")
        o.fill_(gm._sentinel(o))
        plan.append((region, want_dev, want, o))
    torch.cuda.synchronize()
    cache = ipa.PipelineCache(budget)
    results = []
    try:
        for n, (st, action) in enumerate(s.steps):
            r = s.reports[pm.Session.state_key(st)]
            if action == "clear":
                cache.clear()
                m.clear()
            elif action == "borrow":
                L.ipk_cache_get(cache.handle, r.keys[0], None, None, None, None, None)
                m.cache.get(r.keys[0])
            else:
                d, out_type, sid = s.descs[pm.Session.state_key(st)]
                region, _, _, o = plan[n]
                rec = m.call(r, region)
                results.append((n, rec, _drive(ipa, d, c.dev[st["frame"]], sid, out_type, o.data_ptr(), cache, region)))
        torch.cuda.synchronize()
        for n, rec, (rc, flag, mask) in results:
            st, action = s.steps[n]
            region, want_dev, want, o = plan[n]
            what = "%s, %s" % (tag, _describe(n, st, action, region))
            if rc != 0:
                f.errs.append("[status] %s: %d" % (what, rc))
                continue
            if gm._differ(o, want_dev):
                f.errs.append("[parity] %s, %s p=%s: %s" % (what, rec["form"], rec["p"], gm._first_difference(o, want, s.descs[pm.Session.state_key(st)][1])))
            if (mask, flag) != (rec["ops_run"], rec["used_fused"] if region is None else rec["windowed"]):
                f.errs.append("[report] %s: ops_run 0x%02x, flag %d; the model (%s, p=%s): 0x%02x" % (what, mask, flag, rec["form"], rec["p"], rec["ops_run"]))
        keys = sorted(m.shapes)
        got = [bool(L.ipk_cache_contains(cache.handle, key)) for key in keys]
        if got != [m.cache.contains(key) for key in keys]:
            f.errs.append("[keys] %s: %d of %d keys present at the end, in the model %d" % (tag, sum(got), len(keys), len(m.cache.order)))
        if _stats(ipa, cache) != m.cache.stats():                              # every lookup was the drivers' own: hits and misses count here, too
            f.errs.append("[stats] %s: bytes, entries, hits, misses, evictions = %r, the model %r" % (tag, _stats(ipa, cache), m.cache.stats()))
    finally:
        cache.close()


PARAMS = [(case, b) for case in pm.SESSION_CASES for b in range(len(pm.BUDGET_IDS))]


@pytest.mark.parametrize("case,b", PARAMS, ids=["%s-%s" % (pm.SESSION_IDS[pm.SESSION_CASES.index(c)], pm.BUDGET_IDS[b]) for c, b in PARAMS])
def test_a_session_under_a_budget(ipa, orc, case, b):
    c = _case(ipa, orc, case)
    budget = c.session.budgets()[b]
    f = bb.Findings("%s under %s = %d bytes" % (c.cid, pm.BUDGET_IDS[b], budget))
    _replay_observed(ipa, orc, c, budget, f)
    if b in pm.UNOBSERVED:
        _replay_unobserved(ipa, orc, c, budget, f)
    gm._report(f)
