"""Edit sessions on caches too small to hold them, as a model (no GPU).

CacheModel is the byte-budgeted LRU of include/imagepipe_amd.h ("Pipeline::new_cache", ipk_cache_*) and src/pipeline.rs:352-372, written down in plain
Python; it is run against the library's own bookkeeping over seeded random sequences.  SessionModel is the cache traffic of one ipk_pipeline_run_cached
or ipk_pipeline_run_cached_region call, derived on the host alone: from the host-only reports (hashes, sizes, region_gather, takes_fastpath,
resamples_cached_region, the fuses_* and scales_plain reports), the descriptor's source fields and the model's state before the call.  The sessions --
a fixed script of edits and a seeded random tail over the same moves -- are built here, and the conditions that keep them from being vacuous (calls that
resume, calls that evict, keys that are recomputed after an eviction, every form of the region driver at every resume position it can reach) are asserted here from
the model alone.  tests/test_gpu_cache_pressure.py replays the same sessions on real caches and takes everything from this module."""
import ctypes as C
import random
from collections import OrderedDict

import numpy as np
import pytest

import util
import test_gpu_staged_paths as sp
import test_switch_matrix_route as mr
from test_switch_matrix_route import W, H, ON, ALL_ON, CACHED, SOURCES, CASES, CASE_IDS
from test_gpu_switch_matrix import CACHE_CASES                              # importing it needs no GPU

FASTPATH = ("fastpath", 0)                                                      # the RGB8 raster with default ops: 8- and 16-bit outputs take the fast path
SESSION_CASES = CACHE_CASES + [FASTPATH]
SESSION_IDS = [CASE_IDS[CASES.index(c)] if c != FASTPATH else "rgb8-fastpath" for c in SESSION_CASES]


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------
# a. the byte-budgeted LRU
# ---------------------------------------------------------------------------------------------
class CacheModel:
    """`get` refreshes recency and counts a hit or a miss; `contains` does neither; `put` first removes an entry of the same key, then evicts from the
    oldest end until the newcomer fits (an entry larger than the whole budget ends up alone); `clear` drops the entries and keeps the counters"""

    def __init__(self, budget):
        self.budget, self.order, self.bytes = budget, OrderedDict(), 0             # order: key -> bytes, least recently used first
        self.hits = self.misses = self.evictions = 0

    def get(self, key):
        if key not in self.order:
            self.misses += 1
            return False
        self.order.move_to_end(key)
        self.hits += 1
        return True

    def contains(self, key):
        return key in self.order

    def put(self, key, nbytes):
        """-> the keys evicted to make room"""
        if key in self.order:
            self.bytes -= self.order.pop(key)
        gone = []
        while self.bytes + nbytes > self.budget and self.order:
            k, n = self.order.popitem(last=False)
            self.bytes -= n
            self.evictions += 1
            gone.append(k)
        self.order[key] = nbytes
        self.bytes += nbytes
        return gone

    def clear(self):
        self.order.clear()
        self.bytes = 0

    def stats(self):
        return self.bytes, len(self.order), self.hits, self.misses, self.evictions


def test_the_model_is_the_lru_of_the_header():
    """the fixed script of tests/test_cache_contract.py::test_lru_byte_budget, on the model"""
    m = CacheModel(1000)
    for i in range(4):
        m.put(i, 250)
    assert m.stats()[:2] == (1000, 4)
    assert m.get(0) and not m.get(9)
    assert m.put(4, 250) == [1]
    assert m.put(5, 600) == [2, 3, 0] and m.bytes == 850
    assert m.put(5, 100) == [] and m.stats()[:2] == (350, 2)
    assert m.put(6, 5000) == [4, 5] and m.stats()[:2] == (5000, 1)              # larger than the budget: alone
    assert m.put(7, 10) == [6] and m.stats() == (10, 1, 1, 1, 7)
    m.clear()
    assert m.stats() == (0, 0, 1, 1, 7)
    z = CacheModel(0)
    assert z.put(1, 0) == [] and z.put(2, 0) == [] and z.stats()[:2] == (0, 2)    # entries of no bytes fit a budget of none
    assert z.put(3, 1) == [1, 2] and z.put(4, 0) == [3] and z.stats()[:2] == (0, 1)


# ---------------------------------------------------------------------------------------------
# b. the model against the library's bookkeeping
# ---------------------------------------------------------------------------------------------
N_OPS, N_KEYS = 20000, 40
LRU_BUDGETS = [0, 1, 999, 1000, 1001, 1 << 40]


def _lib_stats(L, h):
    b, e, hi, mi, ev = C.c_size_t(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.ipk_cache_stats(h, C.byref(b), C.byref(e), C.byref(hi), C.byref(mi), C.byref(ev)) == 0
    return b.value, e.value, hi.value, mi.value, ev.value


@pytest.mark.parametrize("budget", LRU_BUDGETS)
def test_random_sequences_against_the_librarys_bookkeeping(L, budget):
    """N_OPS seeded operations -- put (sizes 0, 1, the budget, the budget + 1, fractions of it, a key again with another size), get, contains, clear --
    and after every one of them `contains` for every key and all five statistics, library against model"""
    rng = random.Random(util.SEED + 31000 + LRU_BUDGETS.index(budget))
    keys = [bytes([k + 1]) * 32 for k in range(N_KEYS)]
    unit = budget if budget < (1 << 20) else 1000
    sizes = [0, 1, unit, unit + 1, unit // 2, unit // 3, unit // 7 + 1, 2 * unit + 3, 250]
    m = CacheModel(budget)
    h = C.c_void_p()
    assert L.ipk_cache_new(budget, C.byref(h)) == 0
    seen = set()
    try:
        for n in range(N_OPS):
            r = rng.random()
            k = rng.randrange(N_KEYS if r < 0.9 else 4)                          # a tenth of the operations crowd on four keys: repeats with a changed size
            if r < 0.001 or n == N_OPS // 2:
                op = "clear"
                assert L.ipk_cache_clear(h) == 0
                m.clear()
            elif rng.random() < 0.55:
                size = rng.choice(sizes)
                op = "put %d %d" % (k, size)
                assert L.ipk_selftest_cache_put(h, keys[k], size) == 0
                m.put(k, size)
            elif rng.random() < 0.7:
                op = "get %d" % k
                assert L.ipk_cache_get(h, keys[k], None, None, None, None, None) == (0 if m.get(k) else 1), (n, op)
            else:
                op = "contains %d" % k
                assert L.ipk_cache_contains(h, keys[k]) == int(m.contains(k)), (n, op)
            seen.add(op.split()[0])
            assert _lib_stats(L, h) == m.stats(), (n, op)
            assert [L.ipk_cache_contains(h, key) for key in keys] == [int(m.contains(k)) for k in range(N_KEYS)], (n, op)
            assert m.bytes <= budget or len(m.order) == 1, (n, op)
    finally:
        L.ipk_cache_free(h)
    assert seen == {"put", "get", "contains", "clear"}
    if budget:
        assert m.evictions > 100 or budget > (1 << 20)
        assert m.hits > 100 and m.misses > 100


# ---------------------------------------------------------------------------------------------
# c. one driver call's traffic, from the host alone
# ---------------------------------------------------------------------------------------------
SETTINGS = [0, ON, ALL_ON, ON | CACHED]
EXPOSURE_EDIT = 0.5
WB_EDIT = (1.7, 1.0, 1.9, 1.0)                                                 # normalize_wbs leaves it as it is
ORIENT_EDIT = dict(rotation=3, fliph=0, flipv=0)                               # Rotate270: transposing, and neither geometry's own orientation
RC_EDITS = {"crop": (0.05, 0.1, 0.0, 0.07, 0.0), "angle": (0.0, 0.0, 0.0, 0.0, 0.03)}
START = dict(frame=0, exposure=None, wb=None, orient=None, rc=None, out=0, setting=1)
KEY_EPS = 1e-5                                                                 # OpRotateCrop's no-op threshold is far below every value used here


def copy_desc(d):
    return type(d).from_buffer_copy(d)


def base_desc(L, orc, case):
    """the descriptor of a session's first frame, every edit undone and every switch off.  mr.build_desc with the source's own levels, the camera of
    tests/test_gpu_staged_paths.py, normalised white balance and the default curve of a raw source, so that the GPU module can hand the same descriptor
    to the library and its mirror to the oracle.  The fast-path case: an uncropped RGB8 raster with PipelineOps::new(Other)'s fields"""
    if case == FASTPATH:
        d = mr.sr._desc(W, H, "", (0, 0, 0, 0), src_type=2, cpp=3, is_cfa=0, fuse=0)
        d.use_fastpath = 1
        name = "rgb8"
    else:
        d = mr.build_desc(orc, *case)
        name = SOURCES[case[0]]
    d.allow_fused = 0
    if name in mr.RASTERS:
        d.blacklevels[:] = [0.0] * 4
        d.whitelevels[:] = [0.0] * 4
        d.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
        d.cam_to_xyz_normalized[:] = [float(v) for v in np.asarray(orc.const_srgb_d65_43(), np.float32).ravel()]
    else:
        _, src = sp._source(name, 12, 12, 1)
        d.blacklevels[:] = src["blacklevels"]
        d.whitelevels[:] = src["whitelevels"]
        out = (C.c_float * 4)()
        assert L.ipk_normalize_wbs((C.c_float * 4)(*util.WB), out) == 0
        d.wb_coeffs[:] = list(out)
        d.cam_to_xyz_normalized[:] = [float(v) for v in sp._cam4().ravel()]
        d.npoints = 1
        d.points[0], d.points[1] = 0.5, 0.6
    return d


def apply_state(base, st):
    """-> (descriptor, out_type, source_id) of a session state"""
    d = copy_desc(base)
    if st["exposure"] is not None:
        d.exposure = st["exposure"]
    if st["wb"] is not None:
        d.wb_coeffs[:] = st["wb"]
    if st["orient"] is not None:
        d.rotation, d.fliph, d.flipv = st["orient"]["rotation"], st["orient"]["fliph"], st["orient"]["flipv"]
    if st["rc"] is not None:
        d.rotatecrop[:] = RC_EDITS[st["rc"]]
    mr.apply_setting(d, SETTINGS[st["setting"]])
    return d, st["out"], 1 + st["frame"]


def frames_of(case):
    """[(samples, RawImage fields or None)] of a session's two frames: the first is tests/test_gpu_switch_matrix.py's frame of the source"""
    import test_gpu_plain_route as pr
    import test_gpu_switch_matrix as gm
    name = "rgb8" if case == FASTPATH else SOURCES[case[0]]
    seed = util.SEED + 33000 + 16 * SESSION_CASES.index(case)
    first = (pr._image("rgb8", H, W, seed + 1), None) if case == FASTPATH else gm._data(name)
    second = (pr._image(name, H, W, seed + 2), None) if name in mr.RASTERS else sp._source(name, H, W, seed + 2)
    return [first, second]


def oracle_desc(orc, data, d, **kw):
    """the oracle's descriptor with a library descriptor's fields, over `data`"""
    f = dict(cfa=d.cfa.decode(), is_cfa=d.is_cfa, cpp=d.cpp, crops=(d.crop_top, d.crop_right, d.crop_bottom, d.crop_left),
             blacklevels=list(d.blacklevels), whitelevels=list(d.whitelevels), rotatecrop=list(d.rotatecrop),
             cam_to_xyz_normalized=np.array(list(d.cam_to_xyz_normalized), np.float32).reshape(3, 4), wb_coeffs=list(d.wb_coeffs), exposure=d.exposure,
             points=[(d.points[2 * k], d.points[2 * k + 1]) for k in range(d.npoints)], rotation=d.rotation, fliph=bool(d.fliph), flipv=bool(d.flipv),
             maxwidth=d.maxwidth, maxheight=d.maxheight, linear=bool(d.linear), use_fastpath=bool(d.use_fastpath))
    f.update(kw)
    return orc.make_pipeline(data, **f)


class Reports:
    """what the host says about a descriptor and an output type: everything SessionModel reads"""

    def __init__(self, L, orc, d, out_type, source_id):
        buf = C.create_string_buffer(256)
        assert L.ipk_pipeline_hashes(C.byref(d), out_type, source_id, buf) == 0, L.ipk_last_error()
        self.keys = [buf.raw[32 * i: 32 * i + 32] for i in range(8)]
        rc, self.dw, self.dh, self.fw, self.fh = mr._sizes(L, d)
        assert rc == 0
        self.fastpath = L.ipk_pipeline_takes_fastpath(C.byref(d), out_type) == 1
        ask = lambda name: getattr(L, "ipk_pipeline_" + name)(C.byref(d), out_type)
        rep = {n: ask(n) for n in ("fuses_rotatecrop", "fuses_scaledown", "fuses_four_colour", "scales_plain", "resamples_cached_region")}
        assert all(v in (0, 1) for v in rep.values()), rep
        bw, bh, a, b, c = C.c_size_t(), C.c_size_t(), C.c_int64(), C.c_int64(), C.c_int64()
        assert L.ipk_pipeline_region_gather(C.byref(d), out_type, 0, 0, 1, 1, C.byref(bw), C.byref(bh), C.byref(a), C.byref(b), C.byref(c)) == 0
        self.bw, self.bh = bw.value, bh.value
        # the descriptor's source fields
        raw = d.src_type in (0, 1)
        self.mosaic = bool(raw and d.cpp == 1 and d.is_cfa)
        self.mono = int(raw and d.cpp == 1 and not d.is_cfa)
        self.cw, self.ch = d.width - d.crop_left - d.crop_right, d.height - d.crop_top - d.crop_bottom
        scale = orc.calculate_scaling_total(self.cw, self.ch, self.dw, self.dh)[0]
        on = (d.allow_fused & ~(mr.CACHED | mr.SCALED_RC)) != 0                   # bits 5 and 6 are nothing without another bit
        still = all(abs(v) < KEY_EPS for v in d.rotatecrop)
        cfa = d.cfa.decode()
        # the one-launch routes of ipk_pipeline_run_cached's shortcut: raw (a mosaic, nothing between demosaic::full and the point-wise ops; a fourth
        # colour only where fuses_four_colour says so), resample (fuses_rotatecrop), scaledown (fuses_scaledown)
        raw_route = on and self.mosaic and still and scale <= 1.0 and ("E" not in cfa or rep["fuses_four_colour"] == 1)
        self.one_launch = bool(raw_route or rep["fuses_rotatecrop"] == 1 or rep["fuses_scaledown"] == 1)
        # gofloat + demosaic in one pass where OpDemosaic would scale: hash 0 is then never stored
        if not on:
            self.one_pass = False
        elif not raw:
            self.one_pass = scale > 1.0
        elif not self.mosaic:
            self.one_pass = rep["scales_plain"] == 1
        else:
            self.one_pass = scale >= sp._minscale(cfa)
        self.resamples = rep["resamples_cached_region"] == 1
        linear = {0: bool(d.linear), 1: False, 2: True}[out_type]
        curve = not (d.npoints == 0 and abs(np.float32(d.exposure)) < np.float32(0.001))
        turned = orc.transform_orientation(d.rotation, bool(d.fliph), bool(d.flipv)) != orc.OR_NORMAL
        self.pointwise = 0x28 | (curve << 4) | ((not linear) << 6) | (turned << 7)    # bits 3..7 on a rectangle: without the reference's no-ops
        # (width, height, colours) per op; a no-op stores its input, which these rules give the same shape
        self.shapes = [(self.cw, self.ch, 1 if self.mosaic else 4), (self.dw, self.dh, 4), (self.bw, self.bh, 4)] + [(self.bw, self.bh, 3)] * 4 + [
            (self.fw, self.fh, 3)]
        self.nbytes = [w * h * c * 4 for w, h, c in self.shapes]


class SessionModel:
    """a CacheModel and the traffic of the driver calls made on it.  call() -> the record of one call: form, resume position p (-1: nothing memoised
    was used), ops_run, windowed, used_fused, whether it evicted, whether it recomputed a key an eviction had removed"""

    def __init__(self, budget):
        self.cache = CacheModel(budget)
        self.shapes = {}                                                       # every key ever stored -> (w, h, colours, mono)
        self.lost = set()                                                      # stored once, removed by an eviction, not stored again since

    def _put(self, r, i, rec):
        key = r.keys[i]
        if key in self.lost:
            rec["recomputed"] = True
            self.lost.discard(key)
        gone = self.cache.put(key, r.nbytes[i])
        self.lost.update(gone)
        rec["evicted"] = rec["evicted"] or bool(gone)
        self.shapes[key] = r.shapes[i] + (r.mono,)

    def _resume(self, r, upto):
        p = -1
        for i in range(upto):                                                  # every hash is looked up, the last hit wins
            if self.cache.get(r.keys[i]):
                p = i
        return p

    def _run_ops(self, r, p, to, rec):
        """ops p + 1 .. to - 1 of run_cached_ops; -> their bits"""
        mask, i = 0, p + 1
        while i < to:
            if i == 0 and r.one_pass:
                mask |= 3
                self._put(r, 1, rec)
                i = 2
                continue
            mask |= 1 << i
            self._put(r, i, rec)
            i += 1
        return mask

    def call(self, r, region=None):
        rec = dict(form=None, p=None, ops_run=0, windowed=0, used_fused=0, evicted=False, recomputed=False, consults=True, region=region)
        if r.fastpath:
            rec.update(form="cut_fastpath" if region else "fastpath", consults=False)
            return rec
        if region is None:
            p = self._resume(r, 8)
            rec["p"] = p
            if p == -1 and r.one_launch:
                self._put(r, 7, rec)
                rec.update(form="shortcut", ops_run=0xFF, used_fused=1)
            else:
                rec.update(form="staged" if p < 7 else "hit", ops_run=self._run_ops(r, p, 8, rec))
                assert rec["ops_run"] == (0xFF << (p + 1)) & 0xFF
            return rec
        if self.cache.get(r.keys[7]):
            rec.update(form="cut_final", p=7)
            return rec
        if r.resamples and not self.cache.contains(r.keys[2]):
            p = self._resume(r, 2)
            rec.update(form="resample", p=p, windowed=1, ops_run=self._run_ops(r, p, 2, rec) | 4 | r.pointwise)
        else:
            p = self._resume(r, 3)
            rec.update(form="gather", p=p, windowed=1, ops_run=self._run_ops(r, p, 3, rec) | r.pointwise)
        return rec

    def observe(self):
        """the GPU module reads every entry with ipk_cache_get, in ascending order of the keys; a read refreshes recency"""
        return [k for k in sorted(self.shapes) if self.cache.get(k)]

    def clear(self):
        self.cache.clear()                                                     # not an eviction: what it removes is not `lost`


# ---------------------------------------------------------------------------------------------
# d. the sessions
# ---------------------------------------------------------------------------------------------
TAIL = 44
BORROW = 0.2


def session_steps(case):
    """[(state, action)]: action is "small", "big", "whole" or "clear".  The fixed script, then TAIL seeded random steps over the same moves"""
    st = dict(START)
    steps = []

    def go(*actions, **edit):
        st.update(edit)
        steps.extend((dict(st), a) for a in actions)
    go("small")                                                                # 1
    go("big")                                                                  # 2
    go("whole")                                                                # 3
    go("small", "whole", out=1)                                                # (the 8- and 16-bit outputs before any edit: the fast path of the
    go("big", out=2)                                                           # descriptor that has one)
    go("big", "whole", exposure=EXPOSURE_EDIT, out=0)                          # 4
    go("whole", exposure=None)                                                 # 5
    go("small", wb=WB_EDIT)                                                    # 6
    go("small", "big", "whole", orient=ORIENT_EDIT)                            # 7
    go("big", "whole", rc="crop")                                              # 8
    go("small", "whole", rc="angle")
    go("big", "whole", rc=None)                                                # 9
    go("big", "whole", out=1)                                                  # 10
    go("small", "whole", out=2)
    go("whole", "big", out=0, orient=None)
    go("big", "whole", setting=0)                                              # 11
    go("big", "small", "whole", setting=2, rc="angle")
    go("small", "big", "whole", setting=3, rc="crop")
    go("big", setting=3, rc="angle", wb=None)
    go("big", "small", setting=1)
    go("clear", "big", "small")                                                # 12
    go("clear")
    go("whole", setting=2)                                                     # nothing memoised, every switch on: the one-launch shortcut where there is one
    go("clear")
    go("whole", "small", setting=2, rc=None)
    go("big", setting=1, rc="angle")
    go("whole", "small", frame=1)                                              # 13
    go("big", "whole", frame=0)
    # the caller borrows the gofloat buffer (ipk_cache_get on hash 0), which makes it younger than the demosaic buffer: the one way a call comes to
    # resume at p = 0 (test_every_form_is_entered_at_every_resume_position_under_every_budget)
    go("clear")
    go("big", "borrow", setting=3, rc="angle")
    go("big", frame=1)
    go("big", "borrow", frame=0)                                               # resample, p = 0 where the second frame's buffers pushed hash 1 out
    go("big", frame=1)
    go("big", frame=0, setting=1)                                              # gather, p = 0
    go("whole")
    rng = random.Random(util.SEED + 32000 + 7 * SESSION_CASES.index(case))
    moves = [("exposure", [None, EXPOSURE_EDIT]), ("wb", [None, WB_EDIT]), ("orient", [None, ORIENT_EDIT]), ("rc", [None, "crop", "angle"]),
             ("out", [0, 1, 2]), ("setting", [0, 1, 2, 3]), ("frame", [0, 1])]
    for _ in range(TAIL):
        if rng.random() < 0.04:
            go("clear")
        if rng.random() < 0.75:
            field, values = moves[rng.choice([0, 0, 1, 2, 3, 3, 4, 5, 5, 6])]
            st[field] = rng.choice([v for v in values if v != st[field]])
        go(rng.choice(["small", "big", "big", "whole", "whole"]))
        if rng.random() < BORROW:
            go("borrow")
    return steps


class Session:
    """a case's steps with the host's reports for every state: built once per case, shared by the budgets (and by the GPU module)"""

    def __init__(self, L, orc, case):
        self.case, self.steps = case, session_steps(case)
        self.base = base_desc(L, orc, case)
        self.reports, self.descs = {}, {}
        for st, action in self.steps:
            k = self.state_key(st)
            if k not in self.reports:
                d, out_type, sid = apply_state(self.base, st)
                self.descs[k] = (d, out_type, sid)
                self.reports[k] = Reports(L, orc, d, out_type, sid)
        first = self.reports[self.state_key(self.steps[0][0])]
        self.e4, self.e3 = first.nbytes[2], first.nbytes[7]
        off = Reports(L, orc, mr.apply_setting(copy_desc(self.base), 0), 0, 1)
        cold = SessionModel(1 << 40)
        cold.call(off)
        self.cold_bytes = cold.cache.bytes                                     # everything a cold switches-off whole-frame run stores

    @staticmethod
    def state_key(st):
        return tuple(sorted((k, str(v)) for k, v in st.items()))

    def budgets(self):
        return [0, self.e4 - 1, self.e4, self.e4 + self.e3, 2 * self.e4 + self.e3, self.cold_bytes - 1, 1 << 28]

    def regions(self, st):
        r = self.reports[self.state_key(st)]
        return dict(zip(("small", "big"), mr.regions_of(r.fw, r.fh)))

    def replay(self, budget, observe=True):
        """-> (the records of the steps, the model after the last of them).  A record of a "clear" step is None"""
        m = SessionModel(budget)
        recs = []
        for st, action in self.steps:
            if action == "clear":
                m.clear()
                recs.append(None)
            elif action == "borrow":
                m.cache.get(self.reports[self.state_key(st)].keys[0])
                recs.append(None)
            else:
                r = self.reports[self.state_key(st)]
                recs.append(m.call(r, None if action == "whole" else self.regions(st)[action]))
            if observe:
                m.observe()
        return recs, m


BUDGET_IDS = ["0", "E4-1", "E4", "E4+E3", "2E4+E3", "cold-1", "1<<28"]
UNOBSERVED = [2, 3, 4]                                                         # the budgets of the unobserved replay
_SESSIONS = {}


def session(L, orc, case):
    if case not in _SESSIONS:
        _SESSIONS[case] = Session(L, orc, case)
    return _SESSIONS[case]


# ---------------------------------------------------------------------------------------------
# e. conditions on the sessions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SESSION_CASES, ids=SESSION_IDS)
def test_a_session_is_the_script_and_a_tail(L, orc, case):
    s = session(L, orc, case)
    assert len(s.steps) >= 40 + TAIL and TAIL >= 40
    assert len(s.budgets()) == len(BUDGET_IDS) == 7 and s.e4 > 0 and s.e3 > 0 and s.cold_bytes > s.e4
    states = [st for st, _ in s.steps]
    assert {st["out"] for st in states} == {0, 1, 2} and {st["setting"] for st in states} == {0, 1, 2, 3}
    assert {st["rc"] for st in states} == {None, "crop", "angle"} and {st["frame"] for st in states} == {0, 1}
    assert any(a == "clear" for _, a in s.steps)
    for st in states:                                                          # both regions exist in every state, one below 256 pixels and one from there up
        small, big = s.regions(st)["small"], s.regions(st)["big"]
        assert small[2] * small[3] < 256 <= big[2] * big[3]
    # the two frames never share a key, an edit of op k keeps the keys before k
    a, b = dict(START), dict(START, frame=1)
    ka, kb = (Reports(L, orc, *apply_state(s.base, st)).keys for st in (a, b))
    assert not set(ka) & set(kb)
    ke = Reports(L, orc, *apply_state(s.base, dict(START, exposure=EXPOSURE_EDIT))).keys
    assert ke[:4] == ka[:4] and not set(ke[4:]) & set(ka)
    kw = Reports(L, orc, *apply_state(s.base, dict(START, wb=WB_EDIT))).keys
    assert kw[:3] == ka[:3] and not set(kw[3:]) & set(ka)


@pytest.mark.parametrize("case", SESSION_CASES, ids=SESSION_IDS)
def test_the_oracle_takes_every_state_of_a_session(L, orc, case):
    """the oracle's descriptor is the library's, field for field (oracle_desc): it negotiates the sizes the reports give for every state, and the
    session's first descriptor gives the result of the descriptor tests/test_gpu_switch_matrix.py builds for the case"""
    s = session(L, orc, case)
    frames = frames_of(case)
    for k, (d, out_type, sid) in s.descs.items():
        r = s.reports[k]
        assert orc.pipeline_sizes(oracle_desc(orc, frames[sid - 1][0], d)) == ((r.dw, r.dh), (r.fw, r.fh)), (k, r.dw, r.dh, r.fw, r.fh)
    if case == FASTPATH:
        return
    name = SOURCES[case[0]]
    data, src = frames[0]
    crops, ops = mr.case_ops(orc, *case)
    d, _, _ = apply_state(s.base, START)
    for out in (sp.F32, sp.U8, sp.U16):
        if name in mr.RASTERS:
            theirs = orc.make_pipeline(data, crops=crops, **dict(ops, exposure=mr.RASTER_EXPOSURE))
        else:
            theirs = sp._oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=util.WB, cam_to_xyz_normalized=sp._cam4()))
        sp._same(sp._want(orc, oracle_desc(orc, data, d), out), sp._want(orc, theirs, out), "%s %s" % (name, out))


def _counts(recs):
    calls = [r for r in recs if r is not None and r["consults"]]
    return dict(calls=len(calls), resumed=sum(r["p"] >= 0 for r in calls), evicted=sum(r["evicted"] for r in calls),
                recomputed=sum(r["recomputed"] for r in calls))


@pytest.mark.parametrize("observe", [True, False], ids=["observed", "unobserved"])
@pytest.mark.parametrize("case", SESSION_CASES, ids=SESSION_IDS)
def test_every_session_resumes_evicts_and_recomputes(L, orc, case, observe):
    s = session(L, orc, case)
    for b, budget in enumerate(s.budgets()):
        if not observe and b not in UNOBSERVED:
            continue
        recs, m = s.replay(budget, observe)
        n = _counts(recs)
        what = (SESSION_IDS[SESSION_CASES.index(case)], BUDGET_IDS[b], n)
        assert m.cache.bytes <= budget or len(m.cache.order) == 1, what
        if budget == 1 << 28:
            assert m.cache.evictions == 0 and n["evicted"] == 0 and n["recomputed"] == 0, what
        if budget >= s.e4:
            assert 4 * n["resumed"] >= n["calls"], what
        if s.e4 <= budget < (1 << 28):
            assert 4 * n["evicted"] >= n["calls"], what
            assert n["recomputed"] >= 1, what


@pytest.mark.parametrize("observe", [True, False], ids=["observed", "unobserved"])
def test_every_form_is_entered_at_every_resume_position_under_every_budget(L, orc, observe):
    """Over all cases, under every budget: the four forms, the shortcut and the staged run; `resample` with p = -1 and 1, `gather` with p = -1, 1 and 2.
    p = 0 -- hash 0 memoised, hash 1 not -- is asserted under 2 * E4 + E3 and under the cold run's bytes less one alone.  No edit of the script moves
    hash 0 without hash 1 (the settings head the chain), every call that stores hash 0 stores hash 1 straight after it, and every resume looks hash 0
    up before hash 1: hash 0 is never the younger of the two, so the LRU never takes hash 1 and leaves hash 0 -- unless the caller itself borrows the
    gofloat buffer (ipk_cache_get), which the sessions therefore do (the "borrow" steps).  Even then both buffers must first fit together and hash 1
    must go later.  Up to E4 they never fit in these sessions (hash 1 alone is at least E4: OpRotateCrop only shrinks) and at 1 << 28 nothing is ever
    evicted: there p = 0 is asserted NOT to occur.  Under E4 + E3 they fit in the scaled-down cases alone, where the sessions do not reach it."""
    p0 = (4, 5)
    for b in range(len(BUDGET_IDS)):
        if not observe and b not in UNOBSERVED:
            continue
        seen = set()
        for case in SESSION_CASES:
            s = session(L, orc, case)
            recs, _ = s.replay(s.budgets()[b], observe)
            seen |= {(r["form"], r["p"]) for r in recs if r is not None}
        forms = {f for f, _ in seen}
        assert {"cut_fastpath", "cut_final", "resample", "gather", "shortcut", "staged"} <= forms, (BUDGET_IDS[b], forms)
        zero = (0,) if b in p0 else ()
        assert {("resample", p) for p in (-1, 1) + zero} <= seen, (BUDGET_IDS[b], sorted(x for x in seen if x[0] == "resample"))
        assert {("gather", p) for p in (-1, 1, 2) + zero} <= seen, (BUDGET_IDS[b], sorted(x for x in seen if x[0] == "gather"))
        if b not in p0 and b != 3:
            assert not {x for x in seen if x[1] == 0 and x[0] in ("resample", "gather")}, "p = 0 under %s: the reasoning above is wrong" % BUDGET_IDS[b]


def test_totals(L, orc):
    """what the GPU module replays under observation, for the record (shown with -s): the sessions are not a handful of calls"""
    total = dict(calls=0, resumed=0, evicted=0, recomputed=0)
    for case in SESSION_CASES:
        s = session(L, orc, case)
        for budget in s.budgets():
            for k, v in _counts(s.replay(budget)[0]).items():
                total[k] += v
    print("cache-consulting calls replayed over %d cases x 7 budgets: %r" % (len(SESSION_CASES), total))
    assert total["calls"] >= 8000 and min(total["resumed"], total["evicted"], total["recomputed"]) >= total["calls"] // 4, total
