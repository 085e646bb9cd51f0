#!/usr/bin/env python
"""Development tool: what an editor's slider step costs as ipk_pipeline_run_cached_region (cache warm up to the buffer behind OpRotateCrop, then ONE
gather launch over the viewport) against the two things the PARENT build offers for the same edit -- ipk_pipeline_run_cached (resumes at to_lab,
materialises and stores every buffer behind it) plus a 2-D copy of the rectangle, and ipk_pipeline_run_region without a cache (window bits on) -- and
whether the launches that use no gather mode (ipk_pointwise_chain, ipk_pointwise_chain_out) kept the parent's speed.
(tools/preview_regions_probe.py and tools/region_windows_probe.py are the tools of the uncached region routes.)

Frames: 6000 x 4000 RGGB u16 noise, and 8640 x 5760 X-Trans u16 noise -> a preview under maxwidth 2160.  Orientations Normal, Rotate180 (the load walks backwards) and Rotate90 (a transposing one: the plain-rectangle gather launch + orient()), outputs f32
and u8, regions of 1/16 and 1/4 of the area (centred) and the whole area.  Every timed call is an EDIT: the exposure changes from call to call, so the
cached forms never find anything behind the curve.  The new call's region is compared bit for bit with the rectangle of ipk_pipeline_run_cached's
result before anything is timed.  Edit loop: wall clock around the call and a stream synchronise (the cached forms allocate and free device buffers
on the host side, which device events do not see), 3 warm-ups.  Un-moded launches: device events on the launch stream, 5 warm-ups.  The parent build
and this one alternate as child processes of one session on one box; medians over all rounds, the parent's own spread (p95 - median) next to them.
usage: tools/cached_region_probe.py --parent /path/to/libparent.so [--out profiles/r15_cached_region.txt] [--runs 20] [--rounds 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

XTRANS = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
FRAMES = [("RGGB 6000x4000", 6000, 4000, "RGGB", 0), ("X-Trans 8640x5760 -> maxwidth 2160", 8640, 5760, XTRANS, 2160)]
ORIENTS = [("Normal", 0), ("Rotate180", 2), ("Rotate90", 1)]
OUTS = [("f32", 0), ("u8", 1)]
REGIONS = ["1/16 of the area", "1/4 of the area", "the whole area"]
CHAIN_SIZES = [("3.1 MP", 2160, 1440), ("24 MP", 6000, 4000), ("100 MP", 10000, 10000)]


def _regions(fw, fh):
    return [((fw - fw // 4) // 2, (fh - fh // 4) // 2, fw // 4, fh // 4), (fw // 4, fh // 4, fw // 2, fh // 2), (0, 0, fw, fh)]


def _events(run, runs):
    import torch
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def _wall(run, runs, warm=3):
    import torch
    ts = []
    for k in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); run(); torch.cuda.synchronize()
        if k >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def worker(runs, new_build):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case"""
    import torch
    import imagepipe_amd as ipa
    import util
    from imagepipe_amd import _lib
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    cm = (C.c_float * 12)(*[float(v) for v in util.cam_matrix().ravel()])
    wb = (C.c_float * 4)(*util.WB)
    pts = (C.c_float * 2)(0.5, 0.6)
    # ---- the launches that use no mode ----
    for name, w, h in CHAIN_SIZES:
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + w)
        src = torch.rand((w * h, 4), device="cuda", generator=g, dtype=torch.float32)
        src[:, 3] = 0.0
        dst = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
        res = dict(case="chain " + name)
        run = lambda: L.ipk_pointwise_chain(src.data_ptr(), w, h, 0, wb, cm, 0.3, pts, 1, 0, dst.data_ptr(), st)
        for _ in range(5):
            _lib.check(run(), "ipk_pointwise_chain")
        torch.cuda.synchronize()
        res["ipk_pointwise_chain"] = _events(run, 2 * runs)
        if w * h < 50_000_000:
            d8 = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
            run8 = lambda: L.ipk_pointwise_chain_out(src.data_ptr(), w, h, 0, wb, cm, 0.3, pts, 1, 0, 1, d8.data_ptr(), st)
            for _ in range(5):
                _lib.check(run8(), "ipk_pointwise_chain_out")
            torch.cuda.synchronize()
            res["ipk_pointwise_chain_out u8"] = _events(run8, 2 * runs)
            del d8
        print("RESULT " + json.dumps(res), flush=True)
        del src, dst
        torch.cuda.empty_cache()
    # ---- the edit loop ----
    step = [0]

    def edit(pipe):
        step[0] += 1
        pipe.ops.basecurve.exposure = 0.1 + 0.001 * (step[0] % 512)           # a value no earlier call of this process left in the cache

    for name, W, H, cfa, mw in FRAMES:
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + W)
        data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa=cfa, is_float=False, blacklevels=[util.BLACK] * 4,
                                                         whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
        pipe.globals.settings.maxwidth = mw
        pipe.window_regions = pipe.window_previews = True
        for oname, rot in ORIENTS:
            pipe.ops.transform.rotation = rot
            _, (fw, fh) = pipe.sizes()
            for tname, out_type in OUTS:
                dt = torch.float32 if out_type == 0 else torch.uint8
                res = dict(case="%s, %s, %s" % (name, oname, tname), out="%dx%d" % (fw, fh))
                cache = ipa.PipelineCache(6 << 30)
                full = torch.empty(fw * fh * 3, dtype=dt, device="cuda")
                fv = full.view(fh, fw, 3)
                pipe._run(out_type, out=full, cache=cache)                     # warm: with nothing memoised this is the one-launch shortcut ...
                pipe.ops.basecurve.exposure = 0.05
                cache.clear()
                if new_build:
                    pipe.run_region(0, 0, 16, 16, out_type, cache=cache)       # ... so the cache is brought up to op 2 by the new call,
                else:
                    pipe.allow_fused = False; pipe._run(out_type, out=full, cache=cache); pipe.allow_fused = True   # or by a staged run on the parent
                torch.cuda.synchronize()
                for (x, y, w, h), regname in zip(_regions(fw, fh), REGIONS):
                    reg = torch.empty(w * h * 3, dtype=dt, device="cuda")
                    rv = reg.view(h, w, 3)

                    def cached_copy():
                        edit(pipe)
                        pipe._run(out_type, out=full, cache=cache)
                        rv.copy_(fv[y:y + h, x:x + w])

                    def uncached():
                        edit(pipe)
                        pipe.run_region(x, y, w, h, out_type, out=reg)

                    def cached_region():
                        edit(pipe)
                        pipe.run_region(x, y, w, h, out_type, out=reg, cache=cache)

                    if new_build:
                        cached_region(); got = reg.clone(); reg.zero_()        # first: the final buffer of this exposure must not be in the cache yet
                        torch.cuda.synchronize()
                        assert pipe.last_region_windowed and pipe.last_ops_run & 7 == 0, (name, regname, pipe.last_ops_run)
                        step[0] -= 1; cached_copy()
                        torch.cuda.synchronize()
                        assert torch.equal(got.view(torch.uint8), reg.view(torch.uint8)), "%s %s: the region differs from the rectangle of the cached run" % (res["case"], regname)
                        res[regname + "|cached_region"] = _wall(cached_region, runs)
                    res[regname + "|cached+copy"] = _wall(cached_copy, max(runs // 2, 5))
                    assert pipe.last_ops_run & 0x0F == 0, pipe.last_ops_run    # every timed run resumed behind to_lab
                    res[regname + "|uncached"] = _wall(uncached, max(runs // 2, 5))
                    del reg, rv
                print("RESULT " + json.dumps(res), flush=True)
                cache.close()
                del full, fv
                torch.cuda.empty_cache()
        del data, pipe
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_cached_region.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new")
    import numpy as np
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline")
    acc = {}
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
                    r = json.loads(line[7:])
                    c = acc.setdefault(r["case"], dict(out=r.get("out", ""), t={}, rounds={}))
                    for k, v in r.items():
                        if isinstance(v, list):
                            c["t"].setdefault((which, k), []).extend(v)
                            c["rounds"].setdefault((which, k), []).append(float(np.median(v)))
            print("round %d %s done" % (rnd, which), flush=True)
    med = lambda x: float(np.median(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["cached_region_probe: u16 noise frames; %d rounds of (parent build, this build) as alternating child processes on one box; spread = the parent's p95 - median" % a.rounds,
             "", "launches that use no gather mode (device events, %d runs per round, 5 warm-ups); within = this build's median - parent median <= the parent's spread" % (2 * a.runs)]
    ok_all = True
    for case, c in acc.items():
        if not case.startswith("chain "):
            continue
        for key in ("ipk_pointwise_chain", "ipk_pointwise_chain_out u8"):
            if ("parent", key) not in c["t"]:
                continue
            mp, mn, sp = med(c["t"][("parent", key)]), med(c["t"][("new", key)]), spread(c["t"][("parent", key)])
            ok = mn - mp <= sp
            ok_all = ok_all and ok
            lines.append("  %-8s %-28s parent %.4f ms (spread %.4f)  this build %.4f ms  ratio %.3f  %s" % (case[6:], key, mp, sp, mn, mn / mp, "within" if ok else "OUTSIDE the margin"))
            lines.append("      medians per round (one process each): parent %s   this build %s"
                         % tuple(" / ".join("%.4f" % v for v in c["rounds"][(w, key)]) for w in ("parent", "new")))
    lines += ["", "the edit loop: one exposure edit and the region redrawn, wall clock around the call and a synchronise (ms, medians; 3 warm-ups); the cache holds the buffers",
              "up to OpRotateCrop.  parent A = ipk_pipeline_run_cached + a 2-D copy of the rectangle; parent B = ipk_pipeline_run_region without a cache (window bits on);",
              "new = ipk_pipeline_run_cached_region (%d runs per round; A and B %d).  A and B are the parent BUILD's; this build's A / B follow in brackets" % (a.runs, max(a.runs // 2, 5))]
    slower = []
    for case, c in acc.items():
        if case.startswith("chain "):
            continue
        lines.append("  %s (result %s)" % (case, c["out"]))
        for regname in REGIONS:
            A, B = med(c["t"][("parent", regname + "|cached+copy")]), med(c["t"][("parent", regname + "|uncached")])
            An, Bn = med(c["t"][("new", regname + "|cached+copy")]), med(c["t"][("new", regname + "|uncached")])
            N = med(c["t"][("new", regname + "|cached_region")])
            best = min(A, B)
            if not N < best:
                slower.append("%s, %s (new %.3f ms, parent's better alternative %.3f ms)" % (case, regname, N, best))
            lines.append("    %-17s parent A %8.3f (spread %.3f)  parent B %8.3f (spread %.3f)  [this build A %8.3f  B %8.3f]  new %7.3f   x%.1f over A, x%.2f over B"
                         % (regname, A, spread(c["t"][("parent", regname + "|cached+copy")]), B, spread(c["t"][("parent", regname + "|uncached")]), An, Bn, N, A / N, B / N))
    lines += ["", "un-moded launches: " + ("every case within the parent's spread" if ok_all else "NOT every case within the parent's spread"),
              "edits where the new call is not faster than the better of the parent's two alternatives: " + ("none" if not slower else "; ".join(slower))]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
