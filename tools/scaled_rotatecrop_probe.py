#!/usr/bin/env python
"""Development tool: what a straightened frame whose OpDemosaic scales costs under IPK_FUSED_SCALED_ROTATECROP -- two launches: the scaling gofloat +
demosaic pass into the RGBE buffer, then k_fused_resample's 4-channel source mode over it -- against the PARENT build's run of the same descriptor (the
staged ops, every window bit and fuse flag set), whole frames and regions of 1/16 and 1/4 of the area; and what the shared kernel's untouched modes cost
in this build against the parent's (ipk_raw_to_srgb_resampled and ipk_raw_to_srgb_scaled whole frames, the cached rgbe=1 window launch).

Frames (noise): 6000 x 4000 RGGB u16 at rotation 0.02 (negotiates 5999 x 3999) to f32 and to u8; the same under maxwidth 4000 (scale 1.5); 8640 x 5760
X-Trans u16 under maxwidth 2160; a 6000 x 4000 RGB8 raster under maxwidth 3000.  Every case's whole frame is compared with the CPU oracle (--oracle, the
first round's worker of this build) and with the same build's staged run before it is timed, every region with the rectangle of that frame.  Wall clock
around the call and a stream synchronise, 3 warm-ups, medians and minima over all rounds; the parent build, this build and any --variant (a
tools/build_variant.sh library of this tree: the store policy and the table staging of the RGBE output mode) alternate as child processes of one session
on one box; spread = the parent's p95 - median.
usage: tools/scaled_rotatecrop_probe.py --parent /path/to/libparent.so [--variant name=/path/lib.so ...] [--out profiles/r17_scaled_rotatecrop.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

XTRANS = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
ANGLE = 0.02
# name, width, height, filter ("" = an RGB8 raster), maxwidth, out_type
CASES = [("RGGB 6000x4000 u16 -> f32", 6000, 4000, "RGGB", 0, 0), ("RGGB 6000x4000 u16 -> u8", 6000, 4000, "RGGB", 0, 1),
         ("RGGB 6000x4000 u16 -> maxwidth 4000, u8", 6000, 4000, "RGGB", 4000, 1), ("X-Trans 8640x5760 u16 -> maxwidth 2160, u8", 8640, 5760, XTRANS, 2160, 1),
         ("RGB8 raster 6000x4000 -> maxwidth 3000, u8", 6000, 4000, "", 3000, 1)]
REGIONS = ["the whole frame", "1/16 of the area", "1/4 of the area"]


def _regions(fw, fh):
    return [None, ((fw - fw // 4) // 2, (fh - fh // 4) // 2, fw // 4, fh // 4), (fw // 4, fh // 4, fw // 2, fh // 2)]


def _wall(run, runs, warm=3):
    import torch
    ts = []
    for k in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); run(); torch.cuda.synchronize()
        if k >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def _source(ipa, util, W, H, cfa):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + W)
    if cfa:
        data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa=cfa, is_float=False, blacklevels=[util.BLACK] * 4,
                                                         whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    else:
        data = torch.randint(0, 256, (H * W * 3,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(W, H, data, bits=8))
        pipe.ops.basecurve.exposure = 0.3                                  # an edited raster: no fast path
    pipe.window_regions = pipe.window_previews = pipe.fuse_plain = True
    pipe.fuse_rotatecrop = pipe.fuse_scaledown = True
    return data, pipe


def _oracle(util, data, W, H, cfa, mw, out_type):
    import numpy as np
    import oracle as orc
    if cfa:
        host = data.cpu().numpy().view(np.uint16).reshape(H, W)
        desc = orc.make_pipeline(host, cfa=cfa, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                                 cam_to_xyz_normalized=util.cam_matrix(), rotatecrop=(0, 0, 0, 0, ANGLE), maxwidth=mw)
    else:
        desc = orc.make_pipeline(data.cpu().numpy().reshape(H, W, 3), rotatecrop=(0, 0, 0, 0, ANGLE), maxwidth=mw, exposure=0.3)
    return [orc.pipeline_run, orc.pipeline_output_8bit, orc.pipeline_output_16bit][out_type](desc)


def worker(runs, new_build, oracle):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    import util
    ipa.init(0)
    for name, W, H, cfa, mw, out_type in CASES:
        data, pipe = _source(ipa, util, W, H, cfa)
        pipe.globals.settings.maxwidth = mw
        pipe.ops.rotatecrop.rotation = ANGLE
        (dw, dh), (fw, fh) = pipe.sizes()
        dt = torch.float32 if out_type == 0 else torch.uint8
        res = dict(case=name, out="%dx%d" % (fw, fh), demosaic="%dx%d" % (dw, dh))
        whole = torch.empty(fw * fh * 3, dtype=dt, device="cuda")
        pipe._run(out_type, whole)                                          # the staged run of this build: the yardstick for the bits
        torch.cuda.synchronize()
        staged = whole.clone()
        if new_build:
            pipe.fuse_scaled_rotatecrop = True
            res["admitted"] = int(pipe.fuses_scaled_rotatecrop(out_type))
            assert res["admitted"], name
            whole.zero_()
            pipe._run(out_type, whole)
            torch.cuda.synchronize()
            assert pipe.last_used_fused and torch.equal(whole.view(torch.uint8), staged.view(torch.uint8)), "%s: the route's frame differs from the staged run's" % name
            if oracle:
                want = _oracle(util, data, W, H, cfa, mw, out_type)
                got = whole.cpu().numpy().reshape(fh, fw, 3)
                same = np.array_equal(got.view(np.uint32), want.view(np.uint32)) if out_type == 0 else np.array_equal(got, want)
                assert want.shape == got.shape and (same or (out_type == 0 and np.array_equal(np.isnan(got), np.isnan(want)) and
                                                             np.array_equal(got[~np.isnan(got)].view(np.uint32), want[~np.isnan(want)].view(np.uint32)))), \
                    "%s: the route's frame differs from the oracle's" % name
                res["oracle"] = 1
            pipe.fuse_scaled_rotatecrop = False
        ref = staged.view(fh, fw, 3)
        for reg, regname in zip(_regions(fw, fh), REGIONS):
            if reg is None:
                out = whole
                run = lambda: pipe._run(out_type, out)
            else:
                x, y, w, h = reg
                out = torch.empty(w * h * 3, dtype=dt, device="cuda")
                run = lambda: pipe.run_region(x, y, w, h, out_type, out=out)
            if new_build:
                pipe.fuse_scaled_rotatecrop = True
                out.zero_(); run(); torch.cuda.synchronize()
                if reg is not None:
                    assert pipe.last_region_windowed, (name, regname)
                    assert torch.equal(out.view(h, w, 3), ref[y:y + h, x:x + w]) or out_type == 0 and torch.equal(
                        out.view(torch.int32).view(h, w, 3), ref.view(torch.int32).view(fh, fw, 3)[y:y + h, x:x + w]), "%s %s: the region differs" % (name, regname)
                res[regname + "|new"] = _wall(run, runs)
                pipe.fuse_scaled_rotatecrop = False
            res[regname + "|staged"] = _wall(run, max(runs // 2, 5))
        if new_build and cfa == "RGGB" and mw == 0 and out_type == 0:
            # pass 1 on its own: the RGBE output mode writes dw * dh * 16 bytes that pass 2 reads straight back
            buf = torch.empty(dw * dh * 4, dtype=torch.float32, device="cuda")
            res["pass 1 alone|new"] = _wall(lambda: ipa.raw_demosaic_scaled(data, W, 0, 0, W, H, util.BLACK, util.WHITE, cfa, dw, dh, out=buf), runs)
            del buf
        print("RESULT " + json.dumps(res), flush=True)
        del data, pipe, whole, staged, ref
        torch.cuda.empty_cache()
    # ---- the shared kernel's untouched modes ----
    res = dict(case="untouched modes of k_fused_resample (RGGB 6000x4000 u16 -> u8)")
    data, pipe = _source(ipa, util, 6000, 4000, "RGGB")
    rc = pipe.ops.rotatecrop
    rc.crop_top, rc.crop_right, rc.crop_bottom, rc.crop_left, rc.rotation = 0.1, 0.05, 0.2, 0.0, ANGLE
    assert pipe.fuses_rotatecrop(1)
    _, (fw, fh) = pipe.sizes()
    out = torch.empty(fw * fh * 3, dtype=torch.uint8, device="cuda")
    res["ipk_raw_to_srgb_resampled, whole frame|mode"] = _wall(lambda: pipe._run(1, out), runs)
    cache = ipa.PipelineCache(3 << 29)
    pipe.resample_cached = True
    assert pipe.resamples_cached_region(1)
    x, y, w, h = fw // 4, fh // 4, fw // 2, fh // 2
    reg = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
    pipe.run_region(x, y, w, h, 1, out=reg, cache=cache)
    assert not cache.contains(pipe.hashes(1)[2])
    res["the cached rgbe=1 window launch, 1/4 of the area|mode"] = _wall(lambda: pipe.run_region(x, y, w, h, 1, out=reg, cache=cache), runs)
    cache.close()
    pipe.resample_cached = False
    rc.crop_top = rc.crop_right = rc.crop_bottom = rc.rotation = 0.0
    pipe.globals.settings.maxwidth = 3840
    assert pipe.fuses_scaledown(1)
    _, (fw, fh) = pipe.sizes()
    out = torch.empty(fw * fh * 3, dtype=torch.uint8, device="cuda")
    res["ipk_raw_to_srgb_scaled, whole frame (maxwidth 3840)|mode"] = _wall(lambda: pipe._run(1, out), runs)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_scaled_rotatecrop.txt"))
    ap.add_argument("--variant", action="append", default=[], help="name=/path/to/lib.so: a build of this tree with other switches")
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"]); ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new", a.oracle)
    import numpy as np
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline")
    builds = [("parent", os.path.abspath(a.parent)), ("new", None)] + [tuple(v.split("=", 1)) for v in a.variant]
    acc = {}
    for rnd in range(a.rounds):
        for label, so in builds:
            env = dict(os.environ)
            env.pop("IPK_SO_OVERRIDE", None)
            if so:
                env["IPK_SO_OVERRIDE"] = os.path.abspath(so)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "parent" if label == "parent" else "new", "--runs", str(a.runs)]
            if rnd == 0 and label == "new":
                cmd.append("--oracle")
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (label, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault(r["case"], dict(t={}))
                    for k, v in r.items():
                        if isinstance(v, list):
                            c["t"].setdefault((label, k), []).extend(v)
                        elif k != "case":
                            c[k] = max(v, c.get(k, v)) if isinstance(v, int) else v
            print("round %d %s done" % (rnd, label), flush=True)
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    variants = [b[0] for b in builds[2:]]
    lines = ["scaled_rotatecrop_probe: noise frames at rotation %.2f; %d rounds of (%s) as alternating child processes on one box; wall clock around the call and a"
             % (ANGLE, a.rounds, ", ".join(b[0] for b in builds)),
             "synchronise, ms, medians with the fastest run in brackets; %d runs per round (staged runs %d), 3 warm-ups; spread = the parent's p95 - median." % (a.runs, max(a.runs // 2, 5)),
             "parent = the parent build's run of the descriptor (staged ops; fuse_rotatecrop, fuse_scaledown and every window bit set); staged = this build with",
             "IPK_FUSED_SCALED_ROTATECROP clear; new = this build with the bit set (two launches)." +
             ("  Variants of this build (tools/build_variant.sh), new route only: " + ", ".join(variants) if variants else ""), ""]
    slower = []
    for case, c in acc.items():
        if "untouched" in case:
            lines += ["", "  " + case + ": parent -> this build"]
            for (label, k) in sorted(c["t"]):
                if label == "parent":
                    P, N = c["t"][(label, k)], c["t"][("new", k)]
                    inside = abs(med(N) - med(P)) <= spread(P)
                    lines.append("    %-58s %7.3f (%.3f; spread %.3f) -> %7.3f (%.3f)   %s" % (k.split("|")[0], med(P), low(P), spread(P), med(N), low(N),
                                                                                              "inside the parent's spread" if inside else "OUTSIDE the parent's spread"))
            continue
        lines.append("  %s (demosaic %s, result %s; admitted: %s; checked against the oracle: %s)" % (case, c.get("demosaic"), c.get("out"), c.get("admitted", "?"), c.get("oracle", 0)))
        for regname in REGIONS:
            P, S, N = c["t"][("parent", regname + "|staged")], c["t"][("new", regname + "|staged")], c["t"][("new", regname + "|new")]
            if not med(N) < med(P):
                slower.append("%s, %s (new %.3f ms, parent %.3f ms)" % (case, regname, med(N), med(P)))
            extra = "".join("   %s %7.3f (%.3f)" % (v, med(c["t"][(v, regname + "|new")]), low(c["t"][(v, regname + "|new")])) for v in variants)
            lines.append("    %-17s parent %7.3f (%.3f; spread %.3f)  staged %7.3f (%.3f)  new %7.3f (%.3f)   x%.2f over the parent%s"
                         % (regname, med(P), low(P), spread(P), med(S), low(S), med(N), low(N), med(P) / med(N), extra))
        k = "pass 1 alone|new"
        if ("new", k) in c["t"]:
            lines.append("    %-17s ipk_raw_demosaic_scaled: this build %7.3f (%.3f)%s" % ("pass 1 alone", med(c["t"][("new", k)]), low(c["t"][("new", k)]),
                         "".join("   %s %7.3f (%.3f)" % (v, med(c["t"][(v, k)]), low(c["t"][(v, k)])) for v in variants)))
    lines += ["", "cases where the new route is not faster than the parent's run: " + ("none" if not slower else "; ".join(slower)),
              "not measured: 100 MP frames, 16-bit outputs, photo-like data"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
