#!/usr/bin/env python
"""Development tool: what a region of a cropped, straightened or scaled frame costs as a window of the one launch (allow_fused bit 2,
IPK_FUSED_WINDOW_REGIONS / Pipeline.window_regions) against the same ipk_pipeline_run_region without the bit -- the whole result into scratch and a
copy, which is also all the PARENT build can do -- and against the whole-frame run; and whether the whole-frame launches of k_fused_resample, which
now carry the window fields, kept the parent's speed.
(tools/region_probe.py is the plain fused route's region tool and stays as it is; this one covers the fuse_rotatecrop / fuse_scaledown routes.)

Frame: 6000 x 4000 RGGB u16 noise, outputs u8 and f32.  Routes: rotation 0.04 (k_fused_resample's general mode), a 5 % crop per side without an angle
(the crop-only shortcut: the fused Bayer kernel's window form), maxwidth 4000 (scale 1.5: the axis-aligned mode).  Regions: 1920x1080 at the centre
and at the bottom-right corner, 256x256.  Every region is compared bit for bit with the slice of the whole-frame result BEFORE anything is timed.
Device forms: device events on the launch stream, a synchronise behind every timed run, 5 warm-ups.  Host form (ipk_host_pipeline_run_region, page-
locked buffers): wall clock around the synchronous call, and the bytes it uploads (the window ipk_pipeline_region reports, or the whole frame).
The parent build and this one alternate as child processes of one session on one box: parent, this, parent, this, ...; medians over all rounds, the
parent's own spread (p95 - median) next to them.  Accepted: every region with the bit is faster than the parent's run_region (device and host), and
every whole-frame time of this build lies within the parent's spread of the parent's median.
usage: tools/region_windows_probe.py --parent /path/to/libparent.so [--out profiles/r12_region_windows.txt] [--runs 40] [--rounds 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 6000, 4000
WINDOW_BIT = 4
ROUTES = [("rotation 0.04", dict(rotatecrop=(0.0, 0.0, 0.0, 0.0, 0.04))), ("crop 5 %", dict(rotatecrop=(0.05, 0.05, 0.05, 0.05, 0.0))),
          ("maxwidth 4000 (scale 1.5)", dict(maxwidth=4000))]
OUTS = [("u8", 1), ("f32", 0)]
REGIONS = ["1920x1080 centre", "1920x1080 corner", "256x256"]


def _regions(fw, fh):
    return [((fw - 1920) // 2, (fh - 1080) // 2, 1920, 1080), (fw - 1920, fh - 1080, 1920, 1080), ((fw - 256) // 2 | 1, (fh - 256) // 2 | 1, 256, 256)]


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
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per route and output type"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    import util
    from imagepipe_amd import _lib
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + W)
    data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    hs = L.ipk_host_alloc(W * H * 2)
    hr = L.ipk_host_alloc(1920 * 1080 * 3 * 4)
    frame_host = data.cpu().numpy()
    C.memmove(hs, frame_host.ctypes.data, W * H * 2)
    try:
        for rname, ops in ROUTES:
            pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa="RGGB", is_float=False, blacklevels=[util.BLACK] * 4,
                                                             whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
            if "rotatecrop" in ops:
                r = pipe.ops.rotatecrop
                r.crop_top, r.crop_right, r.crop_bottom, r.crop_left, r.rotation = [float(np.float32(x)) for x in ops["rotatecrop"]]
                pipe.fuse_rotatecrop = True
            else:
                pipe.globals.settings.maxwidth = ops["maxwidth"]
                pipe.fuse_scaledown = True
            _, (fw, fh) = pipe.sizes()
            for oname, ot in OUTS:
                dt, esz = {0: (torch.float32, 4), 1: (torch.uint8, 1)}[ot]
                res = dict(case="%s u16->%s" % (rname, oname), out="%dx%d" % (fw, fh))
                full = torch.empty(fw * fh * 3, dtype=dt, device="cuda")
                d0 = pipe.desc()
                used = C.c_int(0)
                whole = lambda: L.ipk_pipeline_run(C.byref(d0), data.data_ptr(), full.data_ptr(), ot, C.byref(used), st)
                for _ in range(5):
                    _lib.check(whole(), "ipk_pipeline_run")
                torch.cuda.synchronize()
                assert used.value == 1, res["case"] + ": the whole-frame run is not the one launch"
                res["whole"] = _time(whole, runs)
                fv = full.view(fh, fw, 3)
                for (x, y, w, h), regname in zip(_regions(fw, fh), REGIONS):
                    reg = torch.empty(w * h * 3, dtype=dt, device="cuda")
                    for bit in ((0, 1) if new_build else (0,)):
                        d = pipe.desc()
                        if bit:
                            d.allow_fused |= WINDOW_BIT
                        win = C.c_int(-1)
                        run = lambda d=d, win=win: L.ipk_pipeline_run_region(C.byref(d), data.data_ptr(), x, y, w, h, reg.data_ptr(), ot, C.byref(win), st)
                        reg.zero_()
                        for _ in range(5):
                            _lib.check(run(), "ipk_pipeline_run_region")
                        torch.cuda.synchronize()
                        assert win.value == bit, "%s %s: bit %d ran with windowed = %d" % (res["case"], regname, bit, win.value)
                        assert torch.equal(fv[y:y + h, x:x + w].contiguous().view(-1).view(torch.uint8), reg.view(torch.uint8)), \
                            "%s %s bit %d: the region differs from the slice of the whole run" % (res["case"], regname, bit)
                        res["%s|dev|%d" % (regname, bit)] = _time(run, runs)
                        # the host form: the same region from page-locked memory
                        sx, sy, sw, sh = (C.c_size_t() for _ in range(4))
                        route = L.ipk_pipeline_region(C.byref(d), ot, x, y, w, h, C.byref(sx), C.byref(sy), C.byref(sw), C.byref(sh))
                        assert route == bit
                        # what the host form uploads: the window's rows widened to 64-byte boundaries of the frame's rows, or the frame
                        b0, b1 = sx.value * 2 // 64 * 64, min(W * 2, (sx.value * 2 + sw.value * 2 + 63) // 64 * 64)
                        res["%s|bytes|%d" % (regname, bit)] = (b1 - b0) * sh.value if route == 1 else W * H * 2
                        hrun = lambda d=d, win=win: L.ipk_host_pipeline_run_region(C.byref(d), hs, x, y, w, h, hr, ot, C.byref(win))
                        for _ in range(3):
                            _lib.check(hrun(), "ipk_host_pipeline_run_region")
                        got = np.ctypeslib.as_array((C.c_uint8 * (w * h * 3 * esz)).from_address(hr))
                        assert np.array_equal(got, fv[y:y + h, x:x + w].contiguous().view(-1).view(torch.uint8).cpu().numpy()), \
                            "%s %s bit %d: the host region differs from the slice of the whole run" % (res["case"], regname, bit)
                        ts = []
                        for _ in range(max(runs // 4, 5)):
                            t0 = time.perf_counter(); hrun(); ts.append(1e3 * (time.perf_counter() - t0))
                        res["%s|host|%d" % (regname, bit)] = ts
                    del reg
                print("RESULT " + json.dumps(res), flush=True)
                del full, fv
                torch.cuda.empty_cache()
    finally:
        L.ipk_host_free(hs); L.ipk_host_free(hr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_region_windows.txt"))
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", which, "--runs", str(a.runs)], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (which, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault(r["case"], dict(out=r["out"], t={}))
                    for k, v in r.items():
                        if k not in ("case", "out"):
                            if isinstance(v, list):
                                c["t"].setdefault((which, k), []).extend(v)
                                c.setdefault("rounds", {}).setdefault((which, k), []).append(float(np.median(v)))
                            else:
                                c["t"][(which, k)] = v
            print("round %d %s done" % (rnd, which), flush=True)
    med = lambda x: float(np.median(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["region_windows_probe: %dx%d RGGB u16 noise frame; device forms: device events on the launch stream, a synchronise behind every timed run, 5 warm-ups;" % (W, H),
             "host form: wall clock around the synchronous call, page-locked buffers; every region equal to the slice of the whole-frame result before it was timed;",
             "%d rounds of (parent build, this build) as alternating child processes, %d runs per case and round (host form: %d); spread = the parent's p95 - median"
             % (a.rounds, a.runs, max(a.runs // 4, 5)), ""]
    ok_whole = ok_regions = True
    lines.append("whole frames (ipk_pipeline_run, the one launch in both builds): accepted = this build's median - parent median <= spread")
    lines.append("(the crop 5 % rows run the fused Bayer kernel's window form, which no build here differs in: they show what two builds of untouched code measure)")
    for case, c in acc.items():
        mp, mn, sp = med(c["t"][("parent", "whole")]), med(c["t"][("new", "whole")]), spread(c["t"][("parent", "whole")])
        ok = mn - mp <= sp
        ok_whole = ok_whole and ok
        lines.append("  %-36s -> %-10s parent %.4f ms (spread %.4f)  this build %.4f ms  ratio %.3f  %s" % (case, c["out"], mp, sp, mn, mn / mp, "accepted" if ok else "NOT accepted"))
        lines.append("      medians per round (one process each): parent %s   this build %s"
                     % tuple(" / ".join("%.4f" % v for v in c["rounds"][(w, "whole")]) for w in ("parent", "new")))
    lines += ["", "regions (ipk_pipeline_run_region): parent = whole result + copy; bit 0 = this build without the bit (the same route); bit 1 = the window launch",
              "accepted = bit 1 median < parent median"]
    for case, c in acc.items():
        fw, fh = [int(v) for v in c["out"].split("x")]
        for regname in REGIONS:
            w, h = (1920, 1080) if regname.startswith("1920") else (256, 256)
            mp, m0, m1 = (med(c["t"][k]) for k in (("parent", regname + "|dev|0"), ("new", regname + "|dev|0"), ("new", regname + "|dev|1")))
            ok = m1 < mp
            ok_regions = ok_regions and ok
            lines.append("  %-36s %-17s parent %.4f ms (spread %.4f)  bit 0 %.4f ms  bit 1 %.4f ms  speed-up %6.2fx  (area ratio %.1f)  %s"
                         % (case, regname, mp, spread(c["t"][("parent", regname + "|dev|0")]), m0, m1, mp / m1, fw * fh / (w * h), "accepted" if ok else "NOT accepted"))
    lines += ["", "host form (ipk_host_pipeline_run_region): time and bytes uploaded"]
    for case, c in acc.items():
        for regname in REGIONS:
            mp, m1 = med(c["t"][("parent", regname + "|host|0")]), med(c["t"][("new", regname + "|host|1")])
            ok = m1 < mp
            ok_regions = ok_regions and ok
            lines.append("  %-36s %-17s parent %.3f ms, %d bytes (spread %.3f)  bit 1 %.3f ms, %d bytes  speed-up %6.2fx  %s"
                         % (case, regname, mp, c["t"][("parent", regname + "|bytes|0")], spread(c["t"][("parent", regname + "|host|0")]), m1,
                            c["t"][("new", regname + "|bytes|1")], mp / m1, "accepted" if ok else "NOT accepted"))
    lines += ["", "whole frames: " + ("every case accepted" if ok_whole else "NOT every case accepted"),
              "regions: " + ("every case accepted" if ok_regions else "NOT every case accepted")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
