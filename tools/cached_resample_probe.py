#!/usr/bin/env python
"""Development tool: what one step of a STRAIGHTEN slider costs as ipk_pipeline_run_cached_region under IPK_FUSED_CACHED_RESAMPLE (the cache warm up to the
demosaic buffer, hash 1; then ONE launch of k_fused_resample's cached-buffer source mode over the viewport, tag rgbe=1) against the two things the
PARENT build offers for the same step -- A: ipk_pipeline_run_cached_region without the bit (OpRotateCrop over the whole frame, stored under a hash
the next step invalidates, then the gather launch), B: ipk_pipeline_run_region without a cache (fuse_rotatecrop and every window bit on).
(tools/cached_region_probe.py is the tool of the edits behind OpRotateCrop; tools/rotatecrop_probe.py and tools/region_windows_probe.py time the
shared kernel's mosaic mode against the parent build.)

Frames: 6000 x 4000 RGGB u16 noise to f32 and to u8, 8640 x 5760 X-Trans u16 noise -> a preview under maxwidth 2160 (u8), a 6000 x 4000 RGB8 raster
(u8).  OpRotateCrop crops 2 % per side; every timed call is an EDIT: the angle changes from call to call, so hash 2 always misses.  The angles are the
first 256 of 0.02 + k * 0.00001 that leave hash 1 as it is: the reference hashes the negotiated demosaic size with the settings, the reverse size fold
runs through OpRotateCrop, and a step that moves that size by a pixel changes EVERY hash -- the whole chain then runs again, with the bit or
without it, and such steps are not what this tool times.  Regions of 1/16 and 1/4 of the area (centred) and the whole area of the smallest result
among those angles.  The new call's region is compared bit for bit with A's for the same angle before anything is timed.  A and the new call keep a
cache each, so neither finds what the other stored, and A's holds the hash-2 buffers of two steps at the most: no timed step finds its angle's buffer.  Wall clock around the call and a stream synchronise (A allocates, stores and evicts
whole-frame buffers on the host side, which device events do not see), 3 warm-ups.  The parent build and this one alternate as child processes of one
session on one box; medians over all rounds, the parent's own spread (p95 - median) next to them.
usage: tools/cached_resample_probe.py --parent /path/to/libparent.so [--out profiles/r16_cached_resample.txt] [--runs 20] [--rounds 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

XTRANS = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
# name, width, height, filter ("" = an RGB8 raster), maxwidth, out_type
CASES = [("RGGB 6000x4000 u16 -> f32", 6000, 4000, "RGGB", 0, 0), ("RGGB 6000x4000 u16 -> u8", 6000, 4000, "RGGB", 0, 1),
         ("X-Trans 8640x5760 u16 -> maxwidth 2160, u8", 8640, 5760, XTRANS, 2160, 1), ("RGB8 raster 6000x4000 -> u8", 6000, 4000, "", 0, 1)]
REGIONS = ["1/16 of the area", "1/4 of the area", "the whole area"]
ANGLE0, ANGLE_STEP, ANGLES, CANDIDATES = 0.02, 0.00001, 256, 20000


def _regions(fw, fh):
    return [((fw - fw // 4) // 2, (fh - fh // 4) // 2, fw // 4, fh // 4), (fw // 4, fh // 4, fw // 2, fh // 2), (0, 0, fw, fh)]


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
    ipa.init(0)
    step = [0]

    angles = []

    def edit(pipe):
        step[0] += 1
        pipe.ops.rotatecrop.rotation = angles[step[0] % len(angles)]

    for name, W, H, cfa, mw, out_type in CASES:
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + W)
        if cfa:
            data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
            pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa=cfa, is_float=False, blacklevels=[util.BLACK] * 4,
                                                             whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
        else:
            data = torch.randint(0, 256, (H * W * 3,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
            pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(W, H, data, bits=8))
            pipe.ops.basecurve.exposure = 0.3                                  # an edited raster: no fast path
        pipe.globals.settings.maxwidth = mw
        rc = pipe.ops.rotatecrop
        rc.crop_top = rc.crop_right = rc.crop_bottom = rc.crop_left = 0.02
        pipe.window_regions = pipe.window_previews = pipe.fuse_plain = True
        pipe.fuse_rotatecrop = True
        rc.rotation = ANGLE0
        h1 = pipe.hashes(out_type)[1]
        del angles[:]
        sizes = []
        for k in range(CANDIDATES):
            rc.rotation = ANGLE0 + ANGLE_STEP * k
            if pipe.hashes(out_type)[1] == h1:
                angles.append(rc.rotation); sizes.append(pipe.sizes()[1])
                if len(angles) == ANGLES:
                    break
        assert len(angles) >= 32, "%s: only %d angles keep hash 1" % (name, len(angles))
        fw, fh = min(s[0] for s in sizes), min(s[1] for s in sizes)
        dt = torch.float32 if out_type == 0 else torch.uint8
        res = dict(case=name, out="%dx%d" % (fw, fh), angles="%d in [%.5f, %.5f]" % (len(angles), angles[0], angles[-1]))
        ncache = ipa.PipelineCache(3 << 29)                                     # the new call's: hashes 0..1, never a hash 2
        rc.rotation = ANGLE0
        # A's cache: hashes 0..1 and room for the hash-2 buffers of two steps, so that no timed step finds the buffer an earlier visit of its angle left
        tmp = ipa.PipelineCache(3 << 29)
        pipe.run_region(0, 0, 16, 16, out_type, cache=tmp)
        (bw, bh), _, _, _ = pipe.region_gather(0, 0, 1, 1, out_type)
        budget = tmp.stats()["bytes"] + bw * bh * 16 * 3 // 2
        tmp.close()
        cache = ipa.PipelineCache(budget)
        pipe.run_region(0, 0, 16, 16, out_type, cache=cache)                    # up to op 2, as the parent does
        if new_build:
            pipe.resample_cached = True
            res["admitted"] = int(pipe.resamples_cached_region(out_type))
            res["uncached one launch"] = int(pipe.fuses_rotatecrop(out_type))
            pipe.run_region(0, 0, 16, 16, out_type, cache=ncache)               # up to op 1, by the new call
            assert not ncache.contains(pipe.hashes(out_type)[2])
            pipe.resample_cached = False
        torch.cuda.synchronize()
        for (x, y, w, h), regname in zip(_regions(fw, fh), REGIONS):
            reg = torch.empty(w * h * 3, dtype=dt, device="cuda")

            def parent_a():
                edit(pipe)
                pipe.run_region(x, y, w, h, out_type, out=reg, cache=cache)

            def parent_b():
                edit(pipe)
                pipe.run_region(x, y, w, h, out_type, out=reg)

            def new():
                edit(pipe)
                pipe.resample_cached = True
                pipe.run_region(x, y, w, h, out_type, out=reg, cache=ncache)
                pipe.resample_cached = False

            if new_build:
                new(); got = reg.clone(); reg.zero_()
                torch.cuda.synchronize()
                assert pipe.last_region_windowed and pipe.last_ops_run & 7 == 4, (name, regname, pipe.last_ops_run)
                step[0] -= 1; parent_a()
                torch.cuda.synchronize()
                assert torch.equal(got.view(torch.uint8), reg.view(torch.uint8)), "%s %s: the resampled region differs from the gather route's" % (name, regname)
                res[regname + "|new"] = _wall(new, runs)
            res[regname + "|A"] = _wall(parent_a, max(runs // 2, 5))
            res[regname + "|B"] = _wall(parent_b, max(runs // 2, 5))
            del reg
        print("RESULT " + json.dumps(res), flush=True)
        cache.close(); ncache.close()
        del data, pipe
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_cached_resample.txt"))
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", which, "--runs", str(a.runs)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (which, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault(r["case"], dict(out=r.get("out", ""), t={}))
                    for k, v in r.items():
                        if isinstance(v, list):
                            c["t"].setdefault((which, k), []).extend(v)
                        elif k in ("admitted", "uncached one launch", "angles"):
                            c[k] = v
            print("round %d %s done" % (rnd, which), flush=True)
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["cached_resample_probe: noise frames; %d rounds of (parent build, this build) as alternating child processes on one box; spread = the parent's p95 - median" % a.rounds,
             "", "one straighten step (the angle changes, hash 2 misses) and the region redrawn, wall clock around the call and a synchronise (ms, medians; 3 warm-ups);",
             "the cache holds the demosaic buffer.  parent A = ipk_pipeline_run_cached_region without the bit (OpRotateCrop over the whole frame, then the gather launch);",
             "parent B = ipk_pipeline_run_region without a cache (fuse_rotatecrop and the window bits on); new = ipk_pipeline_run_cached_region under",
             "IPK_FUSED_CACHED_RESAMPLE (%d runs per round; A and B %d).  A and B are the parent BUILD's; this build's A / B follow in brackets." % (a.runs, max(a.runs // 2, 5)),
             "min: the fastest run of all rounds (a wall clock catches every stall of the host and the driver; where many runs of a case stall, its median does too)"]
    slower = []
    for case, c in acc.items():
        lines.append("  %s (result at least %s; angles %s; the route admitted: %s; B is one launch: %s)"
                     % (case, c["out"], c.get("angles", "?"), c.get("admitted", "?"), c.get("uncached one launch", "?")))
        for regname in REGIONS:
            A, B = med(c["t"][("parent", regname + "|A")]), med(c["t"][("parent", regname + "|B")])
            An, Bn = med(c["t"][("new", regname + "|A")]), med(c["t"][("new", regname + "|B")])
            N = med(c["t"][("new", regname + "|new")])
            if not N < min(A, B):
                slower.append("%s, %s (new %.3f ms, parent's better alternative %.3f ms)" % (case, regname, N, min(A, B)))
            lines.append("    %-17s parent A %8.3f (spread %.3f)  parent B %8.3f (spread %.3f)  [this build A %8.3f  B %8.3f]  new %7.3f   x%.1f over A, x%.2f over B"
                         % (regname, A, spread(c["t"][("parent", regname + "|A")]), B, spread(c["t"][("parent", regname + "|B")]), An, Bn, N, A / N, B / N))
            lA, lB, lN = low(c["t"][("parent", regname + "|A")]), low(c["t"][("parent", regname + "|B")]), low(c["t"][("new", regname + "|new")])
            lines.append("    %-17s min: parent A %8.3f  parent B %8.3f  new %7.3f   x%.1f over A, x%.2f over B" % ("", lA, lB, lN, lA / lN, lB / lN))
    lines += ["", "steps where the new call is not faster than the better of the parent's two alternatives: " + ("none" if not slower else "; ".join(slower))]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
