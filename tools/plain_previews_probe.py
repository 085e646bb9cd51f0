#!/usr/bin/env python
"""Development tool: what a downscaled preview of a monochrome or three-sample raw costs under IPK_FUSED_PLAIN_PREVIEWS -- OpGoFloat + OpDemosaic's
scale_down_opbuf branch as ONE pass over the source (ipk_plain_scale_down: the plain modes of k_raw_scaled_demosaic<T>) -- against the PARENT build's run
of the same descriptor (gofloat into a full-size 16-byte-per-pixel buffer, then k_transform_buffer over it; every bit the parent knows set), whole frames
and regions of 1/16 and 1/4 of the area (bit 3 beside bit 7: windowed); one straightened preview (bits 6 and 7: two launches); and what the carrier
kernel's untouched mosaic mode costs in this build against the parent's.

Frames (noise): 6000 x 4000 mono u16, mono f32, cpp3 u16 and cpp3 f32 under maxwidth 1500 to u8 and to f32 and under maxwidth 400 to u8; mono u16 at
rotation 0.02 under maxwidth 3000 to u8; a 6000 x 4000 RGGB u16 mosaic under maxwidth 400 (scale 15: the general kernel) to u8.  Every case's whole frame
is compared with the CPU oracle (--oracle, the first round's worker of this build) and with the same build's run without the bit before it is timed,
every region with the rectangle of that frame.  Wall clock around the call and a stream synchronise, 3 warm-ups, medians and minima over all rounds; the
parent build and this build alternate as child processes of one session on one box; spread = the parent's p95 - median.
usage: tools/plain_previews_probe.py --parent /path/to/libparent.so [--out profiles/r18_plain_previews.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 6000, 4000
ANGLE = 0.02
KINDS = [("mono", False), ("mono", True), ("cpp3", False), ("cpp3", True)]
# name, kind ("rggb": the carrier kernel's mosaic mode), f32 source, maxwidth, out_type, rotation
CASES = [("%s %s -> maxwidth %d, %s" % (k, "f32" if f else "u16", mw, "f32" if o == 0 else "u8"), k, f, mw, o, 0.0)
         for k, f in KINDS for mw, o in ((1500, 1), (1500, 0), (400, 1))]
CASES += [("mono u16 at rotation %.2f -> maxwidth 3000, u8" % ANGLE, "mono", False, 3000, 1, ANGLE),
          ("RGGB u16 -> maxwidth 400, u8 (the carrier kernel's mosaic mode)", "rggb", False, 400, 1, 0.0)]
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


def _source(ipa, util, kind, is_float, seed):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + seed)
    n = W * H * (3 if kind == "cpp3" else 1)
    if is_float:
        data = torch.rand(n, device="cuda", generator=g, dtype=torch.float32) * 16383.0
    else:
        data = torch.randint(0, 16384, (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa="RGGB" if kind == "rggb" else "", cpp=3 if kind == "cpp3" else 1,
                                                     is_float=is_float, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                                                     cam_to_xyz_normalized=util.cam_matrix()))
    # every bit the parent build knows
    pipe.window_regions = pipe.window_previews = pipe.fuse_plain = pipe.fuse_scaled_rotatecrop = True
    pipe.fuse_rotatecrop = pipe.fuse_scaledown = True
    return data, pipe


def _oracle(util, data, kind, is_float, mw, out_type, angle):
    import numpy as np
    import oracle as orc
    host = data.cpu().numpy()
    host = (host if is_float else host.view(np.uint16)).reshape((H, W, 3) if kind == "cpp3" else (H, W))
    desc = orc.make_pipeline(host, cfa="RGGB" if kind == "rggb" else "", cpp=3 if kind == "cpp3" else 1, blacklevels=[util.BLACK] * 4,
                             whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), rotatecrop=(0, 0, 0, 0, angle), maxwidth=mw)
    return [orc.pipeline_run, orc.pipeline_output_8bit, orc.pipeline_output_16bit][out_type](desc)


def _same_bits(np, got, want, out_type):
    if got.shape != want.shape:
        return False
    if out_type != 0:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def worker(runs, new_build, oracle):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    import util
    ipa.init(0)
    for i, (name, kind, is_float, mw, out_type, angle) in enumerate(CASES):
        data, pipe = _source(ipa, util, kind, is_float, 3 * KINDS.index((kind, is_float)) if kind != "rggb" else 99)
        pipe.globals.settings.maxwidth = mw
        pipe.ops.rotatecrop.rotation = angle
        (dw, dh), (fw, fh) = pipe.sizes()
        dt = torch.float32 if out_type == 0 else torch.uint8
        res = dict(case=name, out="%dx%d" % (fw, fh), demosaic="%dx%d" % (dw, dh))
        whole = torch.empty(fw * fh * 3, dtype=dt, device="cuda")
        pipe._run(out_type, whole)                                          # this build without the new bit: the yardstick for the bits
        torch.cuda.synchronize()
        staged = whole.clone()
        plain = kind != "rggb"
        if new_build:
            pipe.scale_plain = plain
            res["admitted"] = int(pipe.scales_plain(out_type))
            assert res["admitted"] == int(plain), name
            if angle:
                assert pipe.fuses_scaled_rotatecrop(out_type), name
            whole.zero_()
            with ipa.launch_log() as ran:
                pipe._run(out_type, whole)
                torch.cuda.synchronize()
            tagged = [e for e in ran if "k_raw_scaled_demosaic<" in e]
            assert len(tagged) == 1 and ("plain=" in tagged[0]) == plain and not [e for e in ran if "_w8" in e], (name, sorted(ran))
            assert torch.equal(whole.view(torch.uint8), staged.view(torch.uint8)), "%s: the route's frame differs from the run without the bit" % name
            if oracle:
                assert _same_bits(np, whole.cpu().numpy().reshape(fh, fw, 3), _oracle(util, data, kind, is_float, mw, out_type, angle), out_type), \
                    "%s: the route's frame differs from the oracle's" % name
                res["oracle"] = 1
            pipe.scale_plain = False
        ref = staged.view(fh, fw, 3)
        for reg, regname in zip(_regions(fw, fh), REGIONS):
            if reg is not None and (angle or kind == "rggb"):
                continue                                                    # one straightened case and the carrier's cost: whole frames
            if reg is None:
                out = whole
                run = lambda: pipe._run(out_type, out)
            else:
                x, y, w, h = reg
                out = torch.empty(w * h * 3, dtype=dt, device="cuda")
                run = lambda: pipe.run_region(x, y, w, h, out_type, out=out)
            if new_build and plain:
                pipe.scale_plain = True
                out.zero_(); run(); torch.cuda.synchronize()
                if reg is not None:
                    assert pipe.last_region_windowed, (name, regname)
                    assert torch.equal(out.view(torch.uint8).view(h, w, -1), ref[y:y + h, x:x + w].contiguous().view(torch.uint8).view(h, w, -1)), \
                        "%s %s: the region differs" % (name, regname)
                res[regname + "|new"] = _wall(run, runs)
                pipe.scale_plain = False
            res[regname + "|staged"] = _wall(run, runs if not plain else max(runs // 2, 5))
        print("RESULT " + json.dumps(res), flush=True)
        del data, pipe, whole, staged, ref
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_plain_previews.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"]); ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new", a.oracle)
    import numpy as np
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline")
    builds = [("parent", os.path.abspath(a.parent)), ("new", None)]
    acc = {}
    for rnd in range(a.rounds):
        for label, so in builds:
            env = dict(os.environ)
            env.pop("IPK_SO_OVERRIDE", None)
            if so:
                env["IPK_SO_OVERRIDE"] = os.path.abspath(so)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", label, "--runs", str(a.runs)]
            if rnd == 0 and label == "new":
                cmd.append("--oracle")
            # the worker's lines are read as they come, so that a long oracle check still shows progress
            p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            seen = []
            for line in p.stdout:
                seen.append(line)
                if line.startswith("RESULT "):
                    print("  round %d %s: %s" % (rnd, label, json.loads(line[7:])["case"]), flush=True)
            if p.wait() != 0:
                sys.stderr.write("".join(seen))
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (label, p.returncode))
            for line in seen:
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
    lines = ["plain_previews_probe: %d x %d noise frames; %d rounds of (parent, new) as alternating child processes on one box; wall clock around the call and a"
             % (W, H, a.rounds),
             "synchronise, ms, medians with the fastest run in brackets; %d runs per round (runs without the bit %d), 3 warm-ups; spread = the parent's p95 - median." % (a.runs, max(a.runs // 2, 5)),
             "parent = the parent build's run of the descriptor (gofloat, then k_transform_buffer over the full-size buffer; every bit it knows set); staged = this",
             "build with IPK_FUSED_PLAIN_PREVIEWS clear; new = this build with the bit set (one pass; regions windowed under bit 3; the straightened case two",
             "launches under bit 6).", ""]
    slower = []
    for case, c in acc.items():
        if "carrier" in case:
            P, N = c["t"][("parent", REGIONS[0] + "|staged")], c["t"][("new", REGIONS[0] + "|staged")]
            inside = abs(med(N) - med(P)) <= spread(P)
            lines += ["", "  " + case + " (demosaic %s; checked against the oracle: %s): parent -> this build" % (c.get("demosaic"), c.get("oracle", 0)),
                      "    %-17s %7.3f (%.3f; spread %.3f) -> %7.3f (%.3f)   %s" % (REGIONS[0], med(P), low(P), spread(P), med(N), low(N),
                                                                                   "inside the parent's spread" if inside else
                                                                                   ("FASTER than the parent beyond its spread" if med(N) < med(P) else "SLOWER than the parent beyond its spread"))]
            continue
        lines.append("  %s (demosaic %s, result %s; admitted: %s; checked against the oracle: %s)" % (case, c.get("demosaic"), c.get("out"), c.get("admitted", "?"), c.get("oracle", 0)))
        for regname in REGIONS:
            if ("new", regname + "|new") not in c["t"]:
                continue
            P, S, N = c["t"][("parent", regname + "|staged")], c["t"][("new", regname + "|staged")], c["t"][("new", regname + "|new")]
            if not med(N) < med(P) - spread(P):
                slower.append("%s, %s (new %.3f ms, parent %.3f ms, spread %.3f)" % (case, regname, med(N), med(P), spread(P)))
            lines.append("    %-17s parent %7.3f (%.3f; spread %.3f)  staged %7.3f (%.3f)  new %7.3f (%.3f)   x%.2f over the parent"
                         % (regname, med(P), low(P), spread(P), med(S), low(S), med(N), low(N), med(P) / med(N)))
    lines += ["", "cases where the new route is NOT faster than the parent's run beyond the parent's spread: " + ("none" if not slower else "; ".join(slower)),
              "not measured: the host form of the regions, 100 MP frames, 16-bit outputs, photo-like data, regions of the straightened case"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
