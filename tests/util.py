"""Shared helpers for the parity tests: deterministic synthetic frames, bit-level comparison, and buffers that show
stray accesses (Guarded destinations with sentinel bands, Embedded sources with poisoned surroundings)."""
import numpy as np

SEED = 0x1A6E9195
MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(seed, n):
    """n outputs of SplitMix64 started at `seed` (vectorised: output i uses state seed + (i+1)*golden)."""
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        z = (np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)) & MASK
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & MASK
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & MASK
        return z ^ (z >> np.uint64(31))


def noise_u16(seed, h, w, maxval=16383):
    """uniform integers in [0, maxval] -- worst case for LUT locality"""
    r = splitmix64(seed, h * w)
    return (r % np.uint64(maxval + 1)).astype(np.uint16).reshape(h, w)


def smooth_u16(seed, h, w):
    """diagonal gradient ((row+col) mod 4096)*4 + 6-bit noise -- realistic LUT locality (max 16383+63 clipped)"""
    rr, cc = np.meshgrid(np.arange(h, dtype=np.uint32), np.arange(w, dtype=np.uint32), indexing="ij")
    base = ((rr + cc) % 4096) * 4
    n = (splitmix64(seed, h * w) & np.uint64(63)).astype(np.uint32).reshape(h, w)
    return np.minimum(base + n, 16383).astype(np.uint16)


def uniform_f32(seed, n, lo=0.0, hi=1.0):
    r = splitmix64(seed, n)
    u = (r >> np.uint64(40)).astype(np.float64) / float(1 << 24)
    return (lo + (hi - lo) * u).astype(np.float32)


# the synthetic camera of SURVEY.md 8(d)
BLACK, WHITE = 512.0, 16383.0
WB = (2.0, 1.0, 1.5, float("nan"))


def cam_matrix():
    """SRGB_D65_43 with rows scaled so that saturated pixels exceed the white point (exercises the cbrtf path)"""
    m = np.array([[0.4124564, 0.3575761, 0.1804375, 0.0],
                  [0.2126729, 0.7151522, 0.0721750, 0.0],
                  [0.0193339, 0.1191920, 0.9503041, 0.0]], dtype=np.float32)
    return (m * np.array([[1.10], [1.05], [1.20]], dtype=np.float32)).astype(np.float32)


SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1.5, 2.0, 8.0, 1e-3, -1e-3, 0.008856452, 0.0088564521, 0.04045, 0.0031308,
                     1e-30, -1e-30, 1e-40, -1e-40, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.99999994, 1.0000001, 3.4e38,
                     1.17549435e-38, 0.9504700, 1.08883, 0.95047, 255.0, 65535.0, 0.33333334, 0.6, 0.5, 0.49999997, 0.50000006],
                    dtype=np.float32)


def ulp_diff(a, b):
    """max |ulp distance| between two f32 arrays (NaN vs NaN counts as 0, NaN vs number as inf)"""
    a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    if np.any(na != nb):
        return np.inf
    ai = a.view(np.int32).astype(np.int64); bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-2147483648) - ai, ai); bi = np.where(bi < 0, np.int64(-2147483648) - bi, bi)
    d = np.abs(ai - bi); d[na] = 0
    return int(d.max()) if d.size else 0


def assert_bits_equal(got, want, what=""):
    """Bit-exact f32 equality (any NaN == any NaN).  The product's bar is 0 ULP; BASELINE.json allows 1 ULP."""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g = got.ravel().view(np.uint32); w = want.ravel().view(np.uint32)
    both_nan = np.isnan(got.ravel()) & np.isnan(want.ravel())
    bad = (g != w) & ~both_nan
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d samples differ (max %s ULP); first at flat index %d: got %r (0x%08x) want %r (0x%08x)" % (
            what, int(bad.sum()), bad.size, ulp_diff(got, want), i, got.ravel()[i], g[i], want.ravel()[i], w[i]))


# ---------------------------------------------------------------------------------------------
# Buffers that show stray accesses.  The layout and the checks are plain numpy (tests/test_guard_helpers.py runs them without a GPU); Guarded and
# Embedded put them on the device.
# ---------------------------------------------------------------------------------------------
GUARD_BAND = 1024            # elements: one 256-pixel strip is 768 samples of a 3-channel result and 1024 of the 4-channel demosaic result
SENTINELS = {"float32": -7.0, "uint8": 0xA5, "uint16": 0x5A5A}
POISONS = {"float32": 0x7FC00000, "uint16": 0xFFFF}          # bit patterns: a quiet NaN; a sample far above every white level


def guard_layout(n, off=0, band=GUARD_BAND):
    """-> (lo, total): the n elements start at element `lo` of a `total`-element allocation.  The leading band is rounded up to whole groups of 256
    elements (a multiple of 256 bytes for every element type), so the frame sits exactly `off` elements past a 256-byte boundary; at least `band`
    elements lie on both sides."""
    assert n >= 0 and off >= 0 and band >= 1
    lo = -(-band // 256) * 256 + off
    return lo, lo + n + band


def guard_fill(n, dtype, off=0, band=GUARD_BAND):
    """the host image of a fresh guarded allocation: bands AND interior hold the sentinel, so a sample nobody wrote shows up in the comparison"""
    dtype = np.dtype(dtype)
    _, total = guard_layout(n, off, band)
    return np.full(total, SENTINELS[dtype.name], dtype=dtype)


def guard_check(a, n, off=0, band=GUARD_BAND, what=""):
    """`a`: the whole allocation as it is after the run.  Asserts that both bands still hold the sentinel and returns the n interior elements."""
    a = np.asarray(a)
    lo, total = guard_layout(n, off, band)
    assert a.ndim == 1 and a.size == total, (what, a.shape, total)
    s = np.array(SENTINELS[a.dtype.name]).astype(a.dtype)
    front, back = np.flatnonzero(a[:lo] != s), np.flatnonzero(a[lo + n:] != s)
    if front.size or back.size:
        raise AssertionError("%s: the guard bands around the destination were written: %d elements before it (nearest %s elements in front of its "
                             "first), %d behind it (nearest %s elements past its last)" % (
                                 what, front.size, lo - int(front[-1]) if front.size else "-", back.size, int(back[0]) + 1 if back.size else "-"))
    return a[lo: lo + n]


def embed_host(data, off=0, poison=None, band=GUARD_BAND):
    """-> (host array, lo): data's samples, flattened, `off` elements past a 256-byte boundary among poison"""
    flat = np.ascontiguousarray(data).ravel()
    assert flat.dtype.name in POISONS, flat.dtype
    bits = np.dtype("uint32" if flat.dtype == np.float32 else "uint16")
    lo, total = guard_layout(flat.size, off, band)
    host = np.full(total, POISONS[flat.dtype.name] if poison is None else poison, dtype=bits)
    host[lo: lo + flat.size] = flat.view(bits)
    return host.view(flat.dtype), lo


def _np_dtype(dtype):
    """numpy's name for a torch or numpy element type (torch keeps u16 bits in int16)"""
    name = str(dtype).replace("torch.", "")
    return np.dtype({"int16": "uint16"}.get(name, name))


class Guarded:
    """a destination of n elements inside a larger allocation, `off` elements past a 256-byte boundary, with a band of sentinels on both sides;
    the interior holds the sentinel too until it is written"""

    def __init__(self, n, dtype, off=0, band=GUARD_BAND):
        import torch
        self.n, self.off, self.band, self.np_dtype = n, off, band, _np_dtype(dtype)
        self.sentinel = SENTINELS[self.np_dtype.name]
        self.lo, total = guard_layout(n, off, band)
        tdt = {"float32": torch.float32, "uint8": torch.uint8, "uint16": torch.int16}[self.np_dtype.name]
        self.t = torch.full((total,), self.sentinel, dtype=tdt, device="cuda")       # guard_fill's image, made on the device
        assert self.t.data_ptr() % 256 == 0, "the allocator's block does not start on a 256-byte boundary"
        self.ptr = self.t.data_ptr() + self.lo * self.t.element_size()

    def view(self, start=0, count=None):
        """the destination (or `count` of its elements from `start`) as a torch view: what the wrappers that take `out=` or tensors are handed"""
        count = self.n - start if count is None else count
        assert 0 <= start and start + count <= self.n
        return self.t[self.lo + start: self.lo + start + count]

    def whole(self):
        """the allocation as it stands, bands included (host copy)"""
        a = self.t.cpu().numpy()
        return a.view(np.uint16) if self.np_dtype == np.uint16 else a

    def result(self, what=""):
        return guard_check(self.whole(), self.n, self.off, self.band, what)


class Embedded:
    """a source frame inside a larger allocation, `off` elements past a 256-byte boundary, with poison on both sides (f32: NaN, u16: 0xFFFF): a sample
    from outside the frame that enters the arithmetic, even with weight 0, breaks parity"""

    def __init__(self, data, off=0, poison=None, band=GUARD_BAND):
        import torch
        self.host, self.lo = embed_host(data, off, poison, band)
        self.n, self.off = int(np.asarray(data).size), off
        self.t = torch.from_numpy(self.host.view(np.int16) if self.host.dtype == np.uint16 else self.host).cuda()
        assert self.t.data_ptr() % 256 == 0, "the allocator's block does not start on a 256-byte boundary"
        self.ptr = self.t.data_ptr() + self.lo * self.t.element_size()

    def view(self, start=0, count=None):
        count = self.n - start if count is None else count
        assert 0 <= start and start + count <= self.n
        return self.t[self.lo + start: self.lo + start + count]

    def assert_untouched(self, what=""):
        now = self.t.cpu().numpy()
        assert np.array_equal(now.view(np.uint8), self.host.view(np.uint8)), "%s: the source allocation was written" % what
