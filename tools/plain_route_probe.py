#!/usr/bin/env python
"""Development tool: what the frames whose OpDemosaic is a pass-through -- u16 monochrome raws, u16 three-sample raws, cropped RGB8 rasters -- cost as
the one launch ipk_plain_to_srgb (allow_fused bit 4, IPK_FUSED_PLAIN / Pipeline.fuse_plain) against the staged ops they take without the bit, which is
also all the PARENT build can do; what their regions, and those of an uncropped raster, cost as a window of that launch against the whole result and
a copy; and whether ipk_raster_to_srgb, whose six kernels now carry the two runtime modes, kept the parent's speed.
(tools/preview_regions_probe.py is the tool of the downscaled previews, tools/region_windows_probe.py of the rotatecrop / scaledown routes.)

Frames: 6000 x 4000 noise.  Whole frames: mono u16 and cpp3 u16, each to u8 and to f32; RGB8 with 5 % crops per side to u8.  Regions (RGB8 with
non-default ops, and mono u16, to u8): 1/16 of the area, 1/4 of the area, the whole area, device and host forms.  Controls: uncropped RGB8 -> u8 and
RGB16 -> u16 through ipk_pipeline_run and ipk_raster_to_srgb itself (the launch whose kernels changed, its route untouched), and
ipk_pointwise_chain_out (k_raster_chain<Rgbe32>: not an affected symbol, the box reference).  Every result with the bit is compared bit for bit with
the one without BEFORE anything is timed.  Device forms: device events on the launch stream, a synchronise behind every timed run, 5 warm-ups.  Host
form: wall clock around the synchronous call, page-locked buffers, and the bytes it uploads.  The parent build and this one alternate as child
processes of one session on one box: parent, this, parent, this, ...; medians over all rounds, the spread (p95 - median) of each side next to them.
usage: tools/plain_route_probe.py --parent /path/to/libparent.so [--out profiles/r14_plain_route.txt] [--runs 30] [--rounds 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAIN_BIT = 16
W, H = 6000, 4000
REGIONS = ["1/16 of the area", "1/4 of the area", "the whole area"]
OUT_F32, OUT_U8, OUT_U16 = 0, 1, 2
ESZ = {OUT_F32: 4, OUT_U8: 1, OUT_U16: 2}
# (case, source, crops, out type): the whole frames the bit moves
WHOLE = [("mono u16 -> u8", "mono", 0, OUT_U8), ("mono u16 -> f32", "mono", 0, OUT_F32), ("cpp3 u16 -> u8", "cpp3", 0, OUT_U8), ("cpp3 u16 -> f32", "cpp3", 0, OUT_F32),
         ("RGB8, 5% crops per side -> u8", "rgb8", 1, OUT_U8)]
CONTROL = [("uncropped RGB8 -> u8 (ipk_pipeline_run)", "rgb8", OUT_U8), ("uncropped RGB16 -> u16 (ipk_pipeline_run)", "rgb16", OUT_U16)]
REGION_SOURCES = ["rgb8", "mono"]


def _regions(fw, fh):
    return [((fw - fw // 4) // 2, (fh - fh // 4) // 2, fw // 4, fh // 4), (fw // 4, fh // 4, fw // 2, fh // 2), (0, 0, fw, fh)]


def _time(run, runs):
    import torch
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def _pipeline(ipa, util, torch, source, cropped):
    """(pipeline, device data, samples per pixel, bytes per sample)"""
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + len(source))
    spp = 1 if source == "mono" else 3
    if source == "rgb8":
        data = torch.randint(0, 256, (H * W * 3,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    else:
        data = torch.randint(0, 65536 if source == "rgb16" else 16384, (H * W * spp,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    if source in ("rgb8", "rgb16"):
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(W, H, data, bits=8 if source == "rgb8" else 16))
        pipe.ops.basecurve.exposure = 0.5                                     # not the default ops: no fast path
    else:
        pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cpp=spp, cfa="", is_float=False, blacklevels=[util.BLACK] * 4,
                                                         whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    if cropped:
        go = pipe.ops.gofloat
        go.crop_top, go.crop_right, go.crop_bottom, go.crop_left = H // 20, W // 20, H // 20, W // 20
    return pipe, data, spp, 1 if source == "rgb8" else 2


def worker(runs, new_build):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): one JSON line of {key: times}"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    import util
    from imagepipe_amd import _lib
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    tdt = {OUT_F32: torch.float32, OUT_U8: torch.uint8, OUT_U16: torch.int16}
    res = {}
    bits = (0, 1) if new_build else (0,)

    def timed(key, run, what):
        for _ in range(5):
            _lib.check(run(), what)
        torch.cuda.synchronize()
        res[key] = _time(run, runs)

    # whole frames
    for case, source, cropped, out_type in WHOLE:
        pipe, data, _, _ = _pipeline(ipa, util, torch, source, cropped)
        _, (fw, fh) = pipe.sizes()
        outs = []
        for bit in bits:
            d = pipe.desc()
            if bit:
                d.allow_fused |= PLAIN_BIT
                assert L.ipk_pipeline_fuses_plain(C.byref(d), out_type) == 1, case
            out = torch.empty(fw * fh * 3, dtype=tdt[out_type], device="cuda")
            used = C.c_int(-1)
            run = lambda d=d, out=out, used=used: L.ipk_pipeline_run(C.byref(d), data.data_ptr(), out.data_ptr(), out_type, C.byref(used), st)
            timed("%s|whole|%d" % (case, bit), run, "ipk_pipeline_run")
            assert used.value == bit, "%s bit %d: used_fused = %d" % (case, bit, used.value)
            outs.append(out)
        if len(outs) == 2:
            a, b = (o.view(torch.int32) if out_type == OUT_F32 else o for o in outs)
            assert torch.equal(a, b), "%s: the one launch differs from the staged result" % case
        del outs, out, data, pipe
        torch.cuda.empty_cache()
    # controls: the untouched route, the launch itself, the unaffected symbol
    for case, source, out_type in CONTROL:
        pipe, data, _, _ = _pipeline(ipa, util, torch, source, 0)
        d = pipe.desc()
        out = torch.empty(W * H * 3, dtype=tdt[out_type], device="cuda")
        timed(case + "|control", lambda: L.ipk_pipeline_run(C.byref(d), data.data_ptr(), out.data_ptr(), out_type, None, st), "ipk_pipeline_run")
        if source == "rgb8":
            wb, cm, pts = (C.c_float * 4)(*util.WB), (C.c_float * 12)(*[float(v) for v in util.cam_matrix().ravel()]), (C.c_float * 2)(0.5, 0.6)
            timed("ipk_raster_to_srgb RGB8 -> u8, 24 MP|control", lambda: L.ipk_raster_to_srgb(data.data_ptr(), 2, W, H, wb, cm, 0.0, pts, 1, 0, OUT_U8, out.data_ptr(), st),
                  "ipk_raster_to_srgb")
            buf4 = torch.rand(W * H * 4, dtype=torch.float32, device="cuda", generator=None)
            buf4.view(-1, 4)[:, 3] = 0.0
            timed("ipk_pointwise_chain_out f32x4 -> u8, 24 MP (box reference)|control",
                  lambda: L.ipk_pointwise_chain_out(buf4.data_ptr(), W, H, 0, wb, cm, 0.0, pts, 1, 0, OUT_U8, out.data_ptr(), st), "ipk_pointwise_chain_out")
            del buf4
        del out, data, pipe
        torch.cuda.empty_cache()
    # regions, u8
    for source in REGION_SOURCES:
        pipe, data, spp, esz = _pipeline(ipa, util, torch, source, 0)
        nbytes = W * H * spp * esz
        hs = L.ipk_host_alloc(nbytes)
        hr = L.ipk_host_alloc(W * H * 3)
        try:
            host = data.cpu().numpy()
            C.memmove(hs, host.ctypes.data, nbytes)
            del host
            full = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
            d0 = pipe.desc()
            _lib.check(L.ipk_pipeline_run(C.byref(d0), data.data_ptr(), full.data_ptr(), OUT_U8, None, st), "ipk_pipeline_run")
            fv = full.view(H, W, 3)
            for (x, y, w, h), regname in zip(_regions(W, H), REGIONS):
                reg = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
                want = fv[y:y + h, x:x + w].contiguous().view(-1)
                for bit in bits:
                    d = pipe.desc()
                    if bit:
                        d.allow_fused |= PLAIN_BIT
                    win = C.c_int(-1)
                    run = lambda d=d, win=win: L.ipk_pipeline_run_region(C.byref(d), data.data_ptr(), x, y, w, h, reg.data_ptr(), OUT_U8, C.byref(win), st)
                    reg.zero_()
                    key = "%s, %s" % (source, regname)
                    timed("%s|dev|%d" % (key, bit), run, "ipk_pipeline_run_region")
                    assert win.value == bit, "%s bit %d ran with windowed = %d" % (key, bit, win.value)
                    assert torch.equal(want, reg), "%s bit %d: the region differs from the slice of the whole run" % (key, bit)
                    sx, sy, sw, sh = (C.c_size_t() for _ in range(4))
                    route = L.ipk_pipeline_region(C.byref(d), OUT_U8, x, y, w, h, C.byref(sx), C.byref(sy), C.byref(sw), C.byref(sh))
                    assert route == bit
                    px = spp * esz
                    b0, b1 = sx.value * px // 64 * 64, min(W * px, (sx.value * px + sw.value * px + 63) // 64 * 64)
                    res["%s|bytes|%d" % (key, bit)] = (b1 - b0) * sh.value if route == 1 else nbytes
                    hrun = lambda d=d, win=win: L.ipk_host_pipeline_run_region(C.byref(d), hs, x, y, w, h, hr, OUT_U8, C.byref(win))
                    for _ in range(3):
                        _lib.check(hrun(), "ipk_host_pipeline_run_region")
                    got = np.ctypeslib.as_array((C.c_uint8 * (w * h * 3)).from_address(hr))
                    assert np.array_equal(got, want.cpu().numpy()), "%s bit %d: the host region differs from the slice of the whole run" % (key, bit)
                    ts = []
                    for _ in range(max(runs // 4, 5)):
                        t0 = time.perf_counter(); hrun(); ts.append(1e3 * (time.perf_counter() - t0))
                    res["%s|host|%d" % (key, bit)] = ts
                del reg, want
            del full, fv
        finally:
            L.ipk_host_free(hs); L.ipk_host_free(hr)
        del data, pipe
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_plain_route.txt"))
    ap.add_argument("--runs", type=int, default=30); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new")
    import numpy as np
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline (tools/build_variant.sh in a checkout of the parent)")
    t, rounds = {}, {}
    for rnd in range(a.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            env.pop("IPK_SO_OVERRIDE", None)
            if which == "parent":
                env["IPK_SO_OVERRIDE"] = os.path.abspath(a.parent)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", which, "--runs", str(a.runs)], env=env, capture_output=True, text=True, timeout=420)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (which, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    for k, v in json.loads(line[7:]).items():
                        if isinstance(v, list):
                            t.setdefault((which, k), []).extend(v)
                            rounds.setdefault((which, k), []).append(float(np.median(v)))
                        else:
                            t[(which, k)] = v
            print("round %d %s done" % (rnd, which), flush=True)
    med = lambda x: float(np.median(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["plain_route_probe: %d x %d noise frames; device forms: device events on the launch stream, a synchronise behind every timed run, 5 warm-ups;" % (W, H),
             "host form: wall clock around the synchronous call, page-locked buffers; every result with the bit equal to the one without before it was timed;",
             "%d rounds of (parent build, this build) as alternating child processes, %d runs per case and round (host form: %d); spread = p95 - median of that side"
             % (a.rounds, a.runs, max(a.runs // 4, 5)), ""]
    lines.append("control: launches that use neither mode; within the margin = this build's median - parent median <= the parent's spread")
    ok_control = True
    for key in sorted(k for w, k in t if w == "parent" and k.endswith("|control")):
        mp, mn, sp = med(t[("parent", key)]), med(t[("new", key)]), spread(t[("parent", key)])
        ok = mn - mp <= sp
        ok_control = ok_control and ok
        lines.append("  %-68s parent %.4f ms (spread %.4f)  this build %.4f ms (spread %.4f)  ratio %.3f  %s"
                     % (key[:-8], mp, sp, mn, spread(t[("new", key)]), mn / mp, "within" if ok else "OUTSIDE the margin"))
        lines.append("      medians per round (one process each): parent %s   this build %s" % tuple(" / ".join("%.4f" % v for v in rounds[(w, key)]) for w in ("parent", "new")))
    slower = []
    lines += ["", "whole frames (ipk_pipeline_run): parent = the staged ops; bit 0 = this build without the bit (the same route); bit 1 = ipk_plain_to_srgb"]
    for case, _, _, _ in WHOLE:
        kp, k0, k1 = ("parent", case + "|whole|0"), ("new", case + "|whole|0"), ("new", case + "|whole|1")
        if not med(t[k1]) < med(t[kp]):
            slower.append("%s, whole frame" % case)
        lines.append("  %-32s parent %.4f ms (spread %.4f)  bit 0 %.4f ms  bit 1 %.4f ms (spread %.4f)  speed-up %6.2fx"
                     % (case, med(t[kp]), spread(t[kp]), med(t[k0]), med(t[k1]), spread(t[k1]), med(t[kp]) / med(t[k1])))
    lines += ["", "regions to u8, device form (ipk_pipeline_run_region): parent = whole result + copy; bit 1 = the launch over the rectangle"]
    for source in REGION_SOURCES:
        for regname in REGIONS:
            key = "%s, %s" % (source, regname)
            kp, k0, k1 = ("parent", key + "|dev|0"), ("new", key + "|dev|0"), ("new", key + "|dev|1")
            if not med(t[k1]) < med(t[kp]):
                slower.append("%s, device form" % key)
            lines.append("  %-28s parent %.4f ms (spread %.4f)  bit 0 %.4f ms  bit 1 %.4f ms (spread %.4f)  speed-up %6.2fx"
                         % (key, med(t[kp]), spread(t[kp]), med(t[k0]), med(t[k1]), spread(t[k1]), med(t[kp]) / med(t[k1])))
    lines += ["", "regions to u8, host form (ipk_host_pipeline_run_region): time and bytes uploaded"]
    for source in REGION_SOURCES:
        for regname in REGIONS:
            key = "%s, %s" % (source, regname)
            kp, k1 = ("parent", key + "|host|0"), ("new", key + "|host|1")
            if not med(t[k1]) < med(t[kp]):
                slower.append("%s, host form" % key)
            lines.append("  %-28s parent %.3f ms, %d bytes (spread %.3f)  bit 1 %.3f ms, %d bytes (spread %.3f)  speed-up %6.2fx"
                         % (key, med(t[kp]), t[("parent", key + "|bytes|0")], spread(t[kp]), med(t[k1]), t[("new", key + "|bytes|1")], spread(t[k1]), med(t[kp]) / med(t[k1])))
    lines += ["", "control: " + ("every case within the parent's spread" if ok_control else "NOT every case within the parent's spread"),
              "cases where the bit is not faster than the parent: " + ("none" if not slower else "; ".join(slower))]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
