"""ipk_pipeline_run_region on the GPU: every region is bit for bit the same rectangle of ipk_pipeline_run's result (and, on small frames, of
the CPU oracle's), on the windowed route and on the whole-frame route, from device and from host memory."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import util
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
W12 = (XT[0:6] + XT[18:24] + XT[6:12] + XT[24:30] + XT[12:18] + XT[30:36]) * 2 + (XT[18:24] + XT[0:6] + XT[24:30] + XT[6:12] + XT[30:36] + XT[12:18]) * 2
W12 = (W12 * 2)[:144]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ipa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _pipe(ipa, raw, cfa="RGGB", is_float=False, crops=(0, 0, 0, 0), **kw):
    import torch
    h, w = raw.shape[:2]
    data = torch.from_numpy(np.ascontiguousarray(raw, np.float32).ravel()).cuda() if is_float else ipa.upload_u16(raw)
    kw.setdefault("blacklevels", [util.BLACK] * 4); kw.setdefault("whitelevels", [util.WHITE] * 4)
    kw.setdefault("wb_coeffs", util.WB); kw.setdefault("cam_to_xyz_normalized", util.cam_matrix())
    return ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=data, cfa=cfa, is_float=is_float, crops=crops, **kw))


def _host(t, out_type, h, w):
    a = t.cpu().numpy()
    if out_type == 2:
        a = a.view(np.uint16)
    return a.reshape(h, w, 3)


def _same(got, want, out_type, what):
    if out_type == 0:
        assert_bits_equal(got, want, what)
    else:
        assert got.shape == want.shape and np.array_equal(got, want), what


def _check_regions(ipa, pipe, out_type, regions, windowed=True, want=None):
    """every region against the slice of the whole run (computed here unless given)"""
    import torch
    _, (fw, fh) = pipe.sizes()
    if want is None:
        full, _, _ = pipe._run(out_type)
        torch.cuda.synchronize()
        want = _host(full, out_type, fh, fw)
    for x, y, w, h in regions:
        got = pipe.run_region(x, y, w, h, out_type)
        torch.cuda.synchronize()
        assert pipe.last_region_windowed == windowed, (x, y, w, h)
        _same(_host(got, out_type, h, w), want[y:y + h, x:x + w], out_type, "region %r out %d" % ((x, y, w, h), out_type))
    return want


def _strip_regions(fw, fh):
    """widths around the strip geometry (4-pixel lane groups, 256-pixel strips) at odd and even offsets, touching each edge and inside"""
    out = []
    rows = [(0, 5), (fh - 3, 3), (11, 17), (1, 1), (0, fh)]
    for i, wd in enumerate([1, 3, 4, 5, 63, 255, 256, 257, 300]):
        for j, x in enumerate([0, fw - wd, 7, 10, (fw - wd) // 2 | 1]):
            if 0 <= x and x + wd <= fw:
                y, h = rows[(i + j) % len(rows)]
                out.append((x, y, wd, h))
    return out


@pytest.mark.parametrize("cfa", ["RGGB", "GRBG", "GBRG", "BGGR", XT, W12])
@pytest.mark.parametrize("src", ["u16", "u16_odd", "f32"])
def test_region_strip_geometry_all_outputs(ipa, orc, cfa, src):
    sw = 341 if src == "u16_odd" else 342                                   # odd sensor pitch: unaligned u16 rows
    sh, crops = 75, (1, 3, 2, 5)
    raw = util.noise_u16(util.SEED + 90 + sw, sh, sw)
    is_float = src == "f32"
    pipe = _pipe(ipa, raw.astype(np.float32) if is_float else raw, cfa, is_float, crops)
    _, (fw, fh) = pipe.sizes()
    regions = _strip_regions(fw, fh)
    for out_type in (0, 1, 2):
        _check_regions(ipa, pipe, out_type, regions)
    if cfa in ("RGGB", XT):                                                 # small frame: the oracle too
        desc = orc.make_pipeline(raw.astype(np.float32) if is_float else raw, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), crops=crops,
                                 blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix())
        want = orc.pipeline_run(desc)
        for x, y, w, h in regions[::3]:
            assert_bits_equal(pipe.run_region(x, y, w, h).cpu().numpy().reshape(h, w, 3), want[y:y + h, x:x + w], "oracle %r" % ((x, y, w, h),))
        o8 = orc.pipeline_output_8bit(desc)
        o16 = orc.pipeline_output_16bit(desc)
        x, y, w, h = regions[-1]
        assert np.array_equal(_host(pipe.run_region(x, y, w, h, 1), 1, h, w), o8[y:y + h, x:x + w])
        assert np.array_equal(_host(pipe.run_region(x, y, w, h, 2), 2, h, w), o16[y:y + h, x:x + w])


@pytest.mark.parametrize("cfa", ["RGGB", "BGGR", XT])
@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (0, 1)])
def test_region_all_orientations(ipa, orc, cfa, rot, fh):
    sh, sw, crops = 70, 290, (3, 1, 2, 5)
    raw = util.noise_u16(util.SEED + 91, sh, sw)
    pipe = _pipe(ipa, raw, cfa, False, crops)
    pipe.ops.transform.rotation, pipe.ops.transform.fliph = rot, bool(fh)
    _, (fw, fh_) = pipe.sizes()
    regions = [(0, 0, 1, 1), (fw - 1, fh_ - 1, 1, 1), (0, 3, fw, 1), (5, 0, 1, fh_), (3, 5, 40, 30), (fw - 33, fh_ - 21, 33, 21), (0, 0, fw, fh_)]
    for out_type in (0, 1):
        _check_regions(ipa, pipe, out_type, regions)
    desc = orc.make_pipeline(raw, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), crops=crops, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                             wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), rotation=rot, fliph=bool(fh))
    want = orc.pipeline_run(desc)
    x, y, w, h = regions[4]
    assert_bits_equal(pipe.run_region(x, y, w, h).cpu().numpy().reshape(h, w, 3), want[y:y + h, x:x + w], "oracle, orientation")


@pytest.mark.parametrize("case", ["guarded", "exact_division", "no_curve", "curve5", "linear", "generic_f32", "huge_f32"])
def test_region_parameter_variants(ipa, case):
    sh, sw = 40, 600
    raw = util.noise_u16(util.SEED + 92, sh, sw)
    kw, is_float, cfa = {}, case.endswith("f32") or case in ("guarded", "exact_division"), "RGGB"
    src = raw.astype(np.float32)
    if case == "guarded":
        kw = dict(blacklevels=[1.0] * 4)                                     # |black| < range/64: per-pixel guards on
    elif case == "exact_division":
        kw = dict(blacklevels=[0.0] * 4, whitelevels=[1e-30] * 4)
    elif case == "generic_f32":
        cfa = XT
    elif case == "huge_f32":
        src = src * np.float32(1e30)
    pipe = _pipe(ipa, src if is_float else raw, cfa, is_float, **kw)
    if case == "no_curve":
        pipe.ops.basecurve.points, pipe.ops.basecurve.exposure = [], 0.0
    elif case == "curve5":
        pipe.ops.basecurve.points = [(0.0, 0.0), (0.2, 0.15), (0.5, 0.55), (0.8, 0.9), (1.0, 1.0)]
    elif case == "linear":
        pipe.globals.settings.linear = True
    regions = [(0, 0, 600, 3), (1, 2, 299, 7), (255, 5, 257, 9), (597, 30, 3, 10), (100, 0, 400, 40)]
    for out_type in (0, 1, 2):
        _check_regions(ipa, pipe, out_type, regions)


def test_region_halo_specials(ipa):
    """a NaN / inf in the halo column or row reaches the region's edge pixels as in the full run; one two pixels outside changes nothing"""
    sh, sw = 48, 700
    base = util.noise_u16(util.SEED + 93, sh, sw).astype(np.float32)
    x, y, w, h = 301, 11, 260, 20
    clean = _pipe(ipa, base, "RGGB", True)
    want_clean = _check_regions(ipa, clean, 0, [(x, y, w, h)])
    for v in (np.nan, np.inf):
        halo = base.copy()
        halo[y + 3, x - 1] = v; halo[y + 5, x + w] = v; halo[y - 1, x + 7] = v; halo[y + h, x + w - 2] = v
        pipe = _pipe(ipa, halo, "RGGB", True)
        want = _check_regions(ipa, pipe, 0, [(x, y, w, h)])
        assert not np.array_equal(want[y:y + h, x:x + w], want_clean[y:y + h, x:x + w])       # the specials do reach the region
        far = base.copy()
        far[y + 3, x - 2] = v; far[y + 5, x + w + 1] = v; far[y - 2, x + 7] = v; far[y + h + 1, x + 9] = v
        pipe = _pipe(ipa, far, "RGGB", True)
        got = pipe.run_region(x, y, w, h).cpu().numpy().reshape(h, w, 3)
        assert_bits_equal(got, want_clean[y:y + h, x:x + w], "special two pixels outside")


def test_region_whole_frame_routes(ipa):
    import torch
    raw = util.noise_u16(util.SEED + 94, 64, 96)
    regions = [(0, 0, 1, 1), (3, 5, 20, 9), (0, 0, 20, 12)]
    cases = []
    p = _pipe(ipa, raw); p.ops.rotatecrop.crop_top, p.ops.rotatecrop.rotation = 0.1, 0.2; cases.append(p)
    p = _pipe(ipa, raw); p.globals.settings.maxwidth = 40; cases.append(p)
    cases.append(_pipe(ipa, raw, "RGBE"))
    cases.append(_pipe(ipa, raw, ""))                                                      # mono
    p = _pipe(ipa, raw); p.allow_fused = False; cases.append(p)
    rgb = util.noise_u16(util.SEED + 95, 64, 96 * 3).reshape(64, 96, 3)
    cases.append(ipa.Pipeline.new_from_source(ipa.RawImage(width=96, height=64, data=ipa.upload_u16(rgb), cpp=3, blacklevels=[util.BLACK] * 4,
                                                            whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix())))
    r8 = (util.noise_u16(util.SEED + 96, 64, 96 * 3) & 255).astype(np.uint8)
    cases.append(ipa.Pipeline.new_from_source(ipa.OtherImage(96, 64, torch.from_numpy(r8.ravel()).cuda(), bits=8)))
    for pipe in cases:
        _, (fw, fh) = pipe.sizes()
        for out_type in (0, 1, 2):
            _check_regions(ipa, pipe, out_type, [r for r in regions if r[0] + r[2] <= fw and r[1] + r[3] <= fh], windowed=False)


def test_region_refusals_write_nothing(ipa):
    import torch
    pipe = _pipe(ipa, util.noise_u16(util.SEED + 97, 40, 300))
    out = torch.full((30,), -7.0, device="cuda")
    for x, y, w, h in [(0, 0, 0, 1), (299, 0, 2, 1), (0, 39, 1, 2), ((1 << 64) - 1, 0, 2, 1)]:
        with pytest.raises(ipa.IpkError):
            pipe.run_region(x, y, w, h, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("src", ["f32", "u16"])
def test_host_region_reads_only_the_window(ipa, src):
    """the host form: everything outside the reported window is poison (NaN / 65535), the result still equals the clean slice"""
    from imagepipe_amd import _lib
    L = ipa.lib()
    sh, sw = 90, 800
    raw = util.noise_u16(util.SEED + 98, sh, sw)
    host = raw.astype(np.float32) if src == "f32" else raw
    pipe = _pipe(ipa, host, "RGGB", src == "f32", (2, 1, 1, 3))
    d = pipe.desc()
    for out_type, (x, y, w, h) in [(0, (301, 11, 260, 20)), (1, (0, 0, 5, 3)), (2, (500, 70, 296, 17)), (1, (0, 0, 796, 87))]:
        win, (sx, sy, swd, shd) = pipe.region(x, y, w, h, out_type)
        assert win == 1
        poisoned = np.full_like(host, np.nan if src == "f32" else 65535)
        poisoned[sy:sy + shd, sx:sx + swd] = host[sy:sy + shd, sx:sx + swd]
        dt = {0: np.float32, 1: np.uint8, 2: np.uint16}[out_type]
        out = np.zeros((h, w, 3), dt)
        wflag = C.c_int(-1)
        _lib.check(L.ipk_host_pipeline_run_region(C.byref(d), poisoned.ctypes.data, x, y, w, h, out.ctypes.data, out_type, C.byref(wflag)),
                   "ipk_host_pipeline_run_region")
        assert wflag.value == 1
        full, _, _ = pipe._run(out_type)
        _, (fw, fh) = pipe.sizes()
        _same(out, _host(full, out_type, fh, fw)[y:y + h, x:x + w], out_type, "host region %r" % ((x, y, w, h),))
    # the whole-frame route from host memory
    pipe.globals.settings.maxwidth = 300
    d = pipe.desc()
    out = np.zeros((10, 20, 3), np.float32)
    _lib.check(L.ipk_host_pipeline_run_region(C.byref(d), host.ctypes.data, 4, 6, 20, 10, out.ctypes.data, 0, C.byref(wflag)), "host whole route")
    assert wflag.value == 0
    full = pipe.run().numpy()
    assert_bits_equal(out, full[6:16, 4:24], "host whole route")


def test_region_100mp_viewport(ipa):
    """the viewer's case: a 2560x1440 viewport of a 100 MP frame, at the centre and at the bottom-right corner (compared on the device)"""
    import torch
    W = H = 10000
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED)
    data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa="RGGB", is_float=True, blacklevels=[util.BLACK] * 4,
                                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    full = pipe.run().data.view(H, W, 3)
    for x, y in [((W - 2560) // 2, (H - 1440) // 2), (W - 2560, H - 1440)]:
        reg = pipe.run_region(x, y, 2560, 1440)
        assert pipe.last_region_windowed
        assert torch.equal(full[y:y + 1440, x:x + 2560].contiguous().view(torch.int32).ravel(), reg.view(torch.int32)), (x, y)
    del full


def test_cpp_mirror_run_region(ipa, tmp_path):
    """Pipeline::run_region of include/imagepipe_amd.hpp from a program built here"""
    src = tmp_path / "region.cpp"
    src.write_text(r'''
#include "imagepipe_amd.hpp"
#include <cstdio>
#include <fstream>
#include <vector>
int main(int argc, char **argv) {
  using namespace imagepipe;
  check(ipk_init(0), "ipk_init");
  const size_t w = 300, h = 40;
  std::vector<uint16_t> raw(w * h);
  std::ifstream(argv[1], std::ios::binary).read(reinterpret_cast<char *>(raw.data()), raw.size() * 2);
  ImageSource img; img.width = w; img.height = h; img.cfa = "RGGB";
  for (int i = 0; i < 4; ++i) { img.blacklevels[i] = 512.0f; img.whitelevels[i] = 16383.0f; }
  img.wb_coeffs[0] = 2.0f; img.wb_coeffs[1] = 1.0f; img.wb_coeffs[2] = 1.5f;
  const float m[12] = {0.4124564f * 1.10f, 0.3575761f * 1.10f, 0.1804375f * 1.10f, 0, 0.2126729f * 1.05f, 0.7151522f * 1.05f, 0.0721750f * 1.05f, 0,
                       0.0193339f * 1.20f, 0.1191920f * 1.20f, 0.9503041f * 1.20f, 0};
  for (int i = 0; i < 12; ++i) img.cam_to_xyz_normalized[i] = m[i];
  img.data = DeviceArray(raw.data(), raw.size() * 2);
  Pipeline p = Pipeline::new_from_source(std::move(img));
  DeviceArray o = p.run_region(37, 5, 211, 17, IPK_OUT_U8);
  std::vector<uint8_t> v(211 * 17 * 3); o.download(v.data());
  std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(v.data()), v.size());
  std::printf("%d\n", p.last_region_windowed ? 1 : 0);
  return 0;
}
''')
    exe = tmp_path / "region"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "imagepipe_amd"), "-limagepipe_amd", "-Wl,-rpath," + os.path.join(ROOT, "imagepipe_amd")])
    raw = util.noise_u16(util.SEED + 99, 40, 300)
    raw.tofile(tmp_path / "in.u16")
    out = subprocess.run([str(exe), str(tmp_path / "in.u16"), str(tmp_path / "out.u8")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "1"
    pipe = _pipe(ipa, raw)
    want = pipe.run_region(37, 5, 211, 17, ipa.OUT_U8).cpu().numpy()
    assert np.array_equal(np.fromfile(tmp_path / "out.u8", np.uint8), want)
