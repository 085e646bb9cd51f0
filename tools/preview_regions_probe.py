#!/usr/bin/env python
"""Development tool: what a region of a downscaled preview costs as a window of the scaling gofloat + demosaic pass (allow_fused bit 3,
IPK_FUSED_WINDOW_PREVIEWS / Pipeline.window_previews) against the same ipk_pipeline_run_region without the bit -- the whole preview into scratch and a
copy, which is also all the PARENT build can do -- and whether the whole-frame launches of the scale-in-one-pass kernels, which now carry a column
window, kept the parent's speed.
(tools/region_windows_probe.py is the tool of the one-launch rotatecrop / scaledown routes, tools/preview_probe.py times the whole preview call.)

Frames: 8640 x 5760 X-Trans u16 noise -> 2160 x 1440 and 6000 x 4000 RGGB u16 noise -> 1500 x 1000, output u8.  Regions: 1/16 of the area (a quarter
of each side, centred), 1/4 of the area (half of each side, centred) and the whole area.  Every region is compared bit for bit with the slice of the
whole-frame result BEFORE anything is timed.  Device forms: device events on the launch stream, a synchronise behind every timed run, 5 warm-ups.
Host form (ipk_host_pipeline_run_region, page-locked buffers): wall clock around the synchronous call, and the bytes it uploads (the window
ipk_pipeline_region reports, its rows widened to 64 bytes, or the whole frame).  Whole frames: ipk_pipeline_run (u8) and ipk_raw_scaled_demosaic
alone.  The parent build and this one alternate as child processes of one session on one box: parent, this, parent, this, ...; medians over all
rounds, the parent's own spread (p95 - median) next to them.
usage: tools/preview_regions_probe.py --parent /path/to/libparent.so [--out profiles/r13_preview_regions.txt] [--runs 40] [--rounds 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

PREVIEW_BIT = 8
XTRANS = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
FRAMES = [("X-Trans 8640x5760 -> 2160x1440", 8640, 5760, XTRANS, 2160), ("RGGB 6000x4000 -> 1500x1000", 6000, 4000, "RGGB", 1500)]
REGIONS = ["1/16 of the area", "1/4 of the area", "the whole area"]
OUT_U8 = 1


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


def worker(runs, new_build):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per frame"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    import util
    from imagepipe_amd import _lib
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    for name, W, H, cfa, mw in FRAMES:
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + W)
        data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        hs = L.ipk_host_alloc(W * H * 2)
        frame_host = data.cpu().numpy()
        C.memmove(hs, frame_host.ctypes.data, W * H * 2)
        pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa=cfa, is_float=False, blacklevels=[util.BLACK] * 4,
                                                         whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
        pipe.globals.settings.maxwidth = mw
        (dw, dh), (fw, fh) = pipe.sizes()
        hr = L.ipk_host_alloc(fw * fh * 3)
        try:
            res = dict(case=name, out="%dx%d" % (fw, fh), frame_bytes=W * H * 2)
            full = torch.empty(fw * fh * 3, dtype=torch.uint8, device="cuda")
            d0 = pipe.desc()
            whole = lambda: L.ipk_pipeline_run(C.byref(d0), data.data_ptr(), full.data_ptr(), OUT_U8, None, st)
            for _ in range(5):
                _lib.check(whole(), "ipk_pipeline_run")
            torch.cuda.synchronize()
            res["whole"] = _time(whole, runs)
            f4 = torch.empty(dw * dh * 4, dtype=torch.float32, device="cuda")
            op = lambda: L.ipk_raw_scaled_demosaic(data.data_ptr(), 0, W, 0, 0, W, H, util.BLACK, util.WHITE, cfa.encode(), dw, dh, f4.data_ptr(), st)
            for _ in range(5):
                _lib.check(op(), "ipk_raw_scaled_demosaic")
            torch.cuda.synchronize()
            res["op"] = _time(op, runs)
            del f4
            fv = full.view(fh, fw, 3)
            for (x, y, w, h), regname in zip(_regions(fw, fh), REGIONS):
                reg = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
                want = fv[y:y + h, x:x + w].contiguous().view(-1)
                for bit in ((0, 1) if new_build else (0,)):
                    d = pipe.desc()
                    if bit:
                        d.allow_fused |= PREVIEW_BIT
                    win = C.c_int(-1)
                    run = lambda d=d, win=win: L.ipk_pipeline_run_region(C.byref(d), data.data_ptr(), x, y, w, h, reg.data_ptr(), OUT_U8, C.byref(win), st)
                    reg.zero_()
                    for _ in range(5):
                        _lib.check(run(), "ipk_pipeline_run_region")
                    torch.cuda.synchronize()
                    assert win.value == bit, "%s %s: bit %d ran with windowed = %d" % (name, regname, bit, win.value)
                    assert torch.equal(want, reg), "%s %s bit %d: the region differs from the slice of the whole run" % (name, regname, bit)
                    res["%s|dev|%d" % (regname, bit)] = _time(run, runs)
                    sx, sy, sw, sh = (C.c_size_t() for _ in range(4))
                    route = L.ipk_pipeline_region(C.byref(d), OUT_U8, x, y, w, h, C.byref(sx), C.byref(sy), C.byref(sw), C.byref(sh))
                    assert route == bit
                    b0, b1 = sx.value * 2 // 64 * 64, min(W * 2, (sx.value * 2 + sw.value * 2 + 63) // 64 * 64)
                    res["%s|bytes|%d" % (regname, bit)] = (b1 - b0) * sh.value if route == 1 else W * H * 2
                    hrun = lambda d=d, win=win: L.ipk_host_pipeline_run_region(C.byref(d), hs, x, y, w, h, hr, OUT_U8, C.byref(win))
                    for _ in range(3):
                        _lib.check(hrun(), "ipk_host_pipeline_run_region")
                    got = np.ctypeslib.as_array((C.c_uint8 * (w * h * 3)).from_address(hr))
                    assert np.array_equal(got, want.cpu().numpy()), "%s %s bit %d: the host region differs from the slice of the whole run" % (name, regname, bit)
                    ts = []
                    for _ in range(max(runs // 4, 5)):
                        t0 = time.perf_counter(); hrun(); ts.append(1e3 * (time.perf_counter() - t0))
                    res["%s|host|%d" % (regname, bit)] = ts
                del reg
            print("RESULT " + json.dumps(res), flush=True)
            del full, fv
        finally:
            L.ipk_host_free(hs); L.ipk_host_free(hr)
        del data
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_preview_regions.txt"))
    ap.add_argument("--runs", type=int, default=40); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new")
    import numpy as np
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline (tools/build_variant.sh)")
    acc = {}
    for rnd in range(a.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            env.pop("IPK_SO_OVERRIDE", None)
            if which == "parent":
                env["IPK_SO_OVERRIDE"] = os.path.abspath(a.parent)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", which, "--runs", str(a.runs)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (which, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault(r["case"], dict(out=r["out"], frame_bytes=r["frame_bytes"], t={}, rounds={}))
                    for k, v in r.items():
                        if isinstance(v, list):
                            c["t"].setdefault((which, k), []).extend(v)
                            c["rounds"].setdefault((which, k), []).append(float(np.median(v)))
                        elif k not in ("case", "out", "frame_bytes"):
                            c["t"][(which, k)] = v
            print("round %d %s done" % (rnd, which), flush=True)
    med = lambda x: float(np.median(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["preview_regions_probe: u16 noise frames, output u8; device forms: device events on the launch stream, a synchronise behind every timed run, 5 warm-ups;",
             "host form: wall clock around the synchronous call, page-locked buffers; every region equal to the slice of the whole-frame result before it was timed;",
             "%d rounds of (parent build, this build) as alternating child processes, %d runs per case and round (host form: %d); spread = the parent's p95 - median"
             % (a.rounds, a.runs, max(a.runs // 4, 5)), ""]
    ok_whole = True
    lines.append("whole frames: ipk_pipeline_run (u8) and ipk_raw_scaled_demosaic alone; within the margin = this build's median - parent median <= the parent's spread")
    for case, c in acc.items():
        for key, label in (("whole", "ipk_pipeline_run"), ("op", "ipk_raw_scaled_demosaic")):
            mp, mn, sp = med(c["t"][("parent", key)]), med(c["t"][("new", key)]), spread(c["t"][("parent", key)])
            ok = mn - mp <= sp
            ok_whole = ok_whole and ok
            lines.append("  %-32s %-24s parent %.4f ms (spread %.4f)  this build %.4f ms  ratio %.3f  %s" % (case, label, mp, sp, mn, mn / mp, "within" if ok else "OUTSIDE the margin"))
            lines.append("      medians per round (one process each): parent %s   this build %s"
                         % tuple(" / ".join("%.4f" % v for v in c["rounds"][(w, key)]) for w in ("parent", "new")))
    lines += ["", "regions, device form (ipk_pipeline_run_region): parent = whole preview + copy; bit 0 = this build without the bit (the same route); bit 1 = the window launch"]
    slower = []
    for case, c in acc.items():
        for regname in REGIONS:
            mp, m0, m1 = (med(c["t"][k]) for k in (("parent", regname + "|dev|0"), ("new", regname + "|dev|0"), ("new", regname + "|dev|1")))
            if not m1 < mp:
                slower.append("%s, %s, device form" % (case, regname))
            lines.append("  %-32s %-17s parent %.4f ms (spread %.4f)  bit 0 %.4f ms  bit 1 %.4f ms  speed-up %6.2fx"
                         % (case, regname, mp, spread(c["t"][("parent", regname + "|dev|0")]), m0, m1, mp / m1))
    lines += ["", "regions, host form (ipk_host_pipeline_run_region): time and bytes uploaded"]
    for case, c in acc.items():
        for regname in REGIONS:
            mp, m1 = med(c["t"][("parent", regname + "|host|0")]), med(c["t"][("new", regname + "|host|1")])
            if not m1 < mp:
                slower.append("%s, %s, host form" % (case, regname))
            lines.append("  %-32s %-17s parent %.3f ms, %d bytes (spread %.3f)  bit 1 %.3f ms, %d bytes  speed-up %6.2fx"
                         % (case, regname, mp, c["t"][("parent", regname + "|bytes|0")], spread(c["t"][("parent", regname + "|host|0")]), m1,
                            c["t"][("new", regname + "|bytes|1")], mp / m1))
    lines += ["", "whole frames: " + ("every case within the parent's spread" if ok_whole else "NOT every case within the parent's spread"),
              "regions where the bit is not faster than the parent: " + ("none" if not slower else "; ".join(slower))]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
