#!/usr/bin/env python
"""Development tool: what a shoot of thumbnails costs per frame when its frames negotiate DIFFERENT preview sizes under one maxwidth -- landscape and
portrait frames of one camera (Normal / Rotate90 alternating), or two bodies of different aspect ratio.  The PARENT build offers such a caller one thing:
its ipk_pipeline_run_batch_each cuts the run at every such frame, a loop of ipk_pipeline_run, two launches per frame.  This build's call with
IPK_FUSED_BATCH_SIZES keeps the frames in one varied run: ONE sized scaling launch and ONE sized point-wise launch per chunk.  Columns: parent = the parent
build's ipk_pipeline_run_batch_each on the same descriptors (every bit it knows set); sized = this build's call with the bit; first / second = this
build's route 2 on frames that ALL have the first / the second of the two shapes (equal sizes: the launches of bits 9 and 10), whose mean is what the
mixed chunk would cost without wasted blocks -- the sized grid is laid over the largest frame, so the difference is the price of the spread of sizes.
Also the carriers' launches outside the mode in both builds: the single ipk_raw_scaled_demosaic 6000x4000 -> 400x266, ipk_pointwise_chain_out at
2160x1440 and 6000x4000 to u8, the uniform batch, and the equal-size frame-table launches under bits 9 and 10.

Frames (noise, device-resident, 8-bit outputs into one allocation), each at n = 2, 8, 16, 64.  Before anything is timed the new call is compared with this
build's loop of ipk_pipeline_run (all frames, equal bytes); the plan must say route 2 and the launch log must show the sized launches.  Wall clock around
the call and a stream synchronise, 3 warm-ups, medians and minima over all rounds; the parent build and this build alternate as child processes of one
session on one box; spread = the parent's p95 - median.
usage: tools/batch_sizes_probe.py --parent /path/to/libparent.so [--out profiles/r24_batch_sizes.txt]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_sensor_probe import _wall, _pipe, _wb, _levels                  # noqa: E402

ORIENTED, SENSOR, SIZES = 512, 1024, 2048
OLD_BITS = 255 | 256 | ORIENTED | SENSOR                                   # every bit the parent knows
# name, [(width, height, rotation), ...] (frame i takes entry i mod 2), maxwidth
CASES = [("24 MP RGGB u16, Normal / Rotate90 alternating -> maxwidth 256 (256x170 beside 384x256)", [(6000, 4000, 0), (6000, 4000, 1)], 256),
         ("24 MP RGGB u16, Normal / Rotate90 alternating -> maxwidth 400 (400x266 beside 600x400)", [(6000, 4000, 0), (6000, 4000, 1)], 400),
         ("24 MP 3:2 / 21 MP 4:3 RGGB u16 alternating -> maxwidth 256 (256x170 beside 256x192)", [(6000, 4000, 0), (5328, 4000, 0)], 256)]
NS = [2, 8, 16, 64]
UNTOUCHED = ["ipk_raw_scaled_demosaic 6000x4000 -> 400x266", "ipk_pointwise_chain_out 2160x1440 to u8", "ipk_pointwise_chain_out 6000x4000 to u8",
             "uniform batch, 24 MP -> 256 wide, n = 16", "bit 9, equal sizes (23 MP under a 256 box, four rotations), n = 16",
             "bit 10, equal sizes (own levels), 24 MP -> 256 wide, n = 16"]


def untouched(runs, ipa, util, L, _lib, frames):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    w, h = 6000, 4000
    dst = torch.empty(400 * 266 * 4, dtype=torch.float32, device="cuda")
    run = lambda: _lib.check(L.ipk_raw_scaled_demosaic(frames[0].data_ptr(), 0, w, 0, 0, w, h, util.BLACK, util.WHITE, b"RGGB", 400, 266, dst.data_ptr(), st),
                             "ipk_raw_scaled_demosaic")
    print("RESULT " + json.dumps({"case": UNTOUCHED[0], "n": -1, "single": _wall(run, 2 * runs)}), flush=True)
    cm = (C.c_float * 12)(*[float(v) for v in util.cam_matrix().ravel()])
    wb = (C.c_float * 4)(*[float(v) for v in util.WB])
    pts = (C.c_float * 2)(0.5, 0.6)
    for name, (cw, ch) in ((UNTOUCHED[1], (2160, 1440)), (UNTOUCHED[2], (6000, 4000))):
        src = torch.rand(cw * ch * 4, device="cuda"); src[3::4] = 0.0
        out = torch.empty(cw * ch * 3, dtype=torch.uint8, device="cuda")
        run = lambda: _lib.check(L.ipk_pointwise_chain_out(src.data_ptr(), cw, ch, 0, wb, cm, 0.0, pts, 1, 0, 1, out.data_ptr(), st), "ipk_pointwise_chain_out")
        print("RESULT " + json.dumps({"case": name, "n": -1, "single": _wall(run, 2 * runs)}), flush=True)
        del src, out
    n = 16
    for name, mode in ((UNTOUCHED[3], "uniform"), (UNTOUCHED[4], "bit9"), (UNTOUCHED[5], "bit10")):
        descs = []
        for i in range(n):
            pipe = _pipe(ipa, util, "RGGB", w, h, 256, frames[i])
            if mode == "bit9":
                pipe.globals.settings.maxheight = 256
                pipe.ops.transform.rotation = i % 4
            d = _lib.PipelineDesc.from_buffer_copy(pipe.desc())
            d.allow_fused = OLD_BITS
            if mode == "bit10":
                b, wl = _levels(util, i)
                d.blacklevels[:] = [b] * 4
                d.whitelevels[:] = [wl] * 4
            if mode != "uniform":
                d.wb_coeffs[:] = _wb(util, i)
            (dw, dh), (fw, fh) = pipe.sizes()
            descs.append(d)
        px3 = fw * fh * 3
        out = torch.zeros(n * px3, dtype=torch.uint8, device="cuda")
        dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs])
        sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
        op = (C.c_void_p * n)(*[out.data_ptr() + i * px3 for i in range(n)])
        route = (C.c_int * n)()
        _lib.check(L.ipk_pipeline_batch_each_plan(dp, n, 1, route, None), "ipk_pipeline_batch_each_plan")
        assert list(route) == [1 if mode == "uniform" else 2] * n, (name, list(route))
        run = lambda: _lib.check(L.ipk_pipeline_run_batch_each(dp, sp, op, n, 1, None, st), "ipk_pipeline_run_batch_each")
        with ipa.launch_log() as ran:
            run(); torch.cuda.synchronize()
        assert not [e for e in ran if "sized=1" in e], sorted(ran)
        print("RESULT " + json.dumps({"case": name, "n": -1, "single": _wall(run, runs)}), flush=True)


def worker(runs, new_build, untouched_only=False):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case and batch size"""
    import torch
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    import util
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    for ci, (name, shapes, mw) in enumerate(CASES):
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 240 + ci)
        frames = [torch.randint(0, 16384, (shapes[i % 2][0] * shapes[i % 2][1],), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
                  for i in range(max(NS))]
        if ci == 0:
            untouched(runs, ipa, util, L, _lib, frames)
            if untouched_only:
                return

        def build(pick):
            """descriptors of frames whose shape is shapes[pick(i)]; frame i keeps its own buffer where the sensor size allows, else frame pick(i)'s"""
            descs, sizes, ptrs = [], [], []
            for i in range(max(NS)):
                w, h, rot = shapes[pick(i)]
                j = i if frames[i].numel() == w * h else pick(i)
                pipe = _pipe(ipa, util, "RGGB", w, h, mw, frames[j])
                pipe.ops.transform.rotation = rot
                (dw, dh), (fw, fh) = pipe.sizes()
                d = _lib.PipelineDesc.from_buffer_copy(pipe.desc())
                d.wb_coeffs[:] = _wb(util, i)
                descs.append(d); sizes.append((dw, dh, fw * fh * 3)); ptrs.append(frames[j].data_ptr())
            return descs, sizes, ptrs

        def each(descs, sizes, ptrs, n, out):
            offs = [sum(s[2] for s in sizes[:i]) for i in range(n)]
            dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
            sp = (C.c_void_p * n)(*ptrs[:n])
            op = (C.c_void_p * n)(*[out.data_ptr() + o for o in offs])
            return dp, lambda: _lib.check(L.ipk_pipeline_run_batch_each(dp, sp, op, n, 1, None, st), "ipk_pipeline_run_batch_each")
        mixed = build(lambda i: i % 2)
        for n in NS:
            descs, sizes, ptrs = mixed
            res = dict(case=name, n=n, demosaic="%dx%d, %dx%d" % (sizes[0][:2] + sizes[1][:2]))
            total = sum(s[2] for s in sizes[:n])
            out = torch.zeros(total, dtype=torch.uint8, device="cuda")
            for d in descs:
                d.allow_fused = OLD_BITS | (SIZES if new_build else 0)
            dp, run = each(descs, sizes, ptrs, n, out)
            if not new_build:
                res["parent"] = _wall(run, runs)
            else:
                pos = 0
                for i in range(n):
                    _lib.check(L.ipk_pipeline_run(C.byref(descs[i]), ptrs[i], out.data_ptr() + pos, 1, None, st), "ipk_pipeline_run")
                    pos += sizes[i][2]
                torch.cuda.synchronize()
                want = out.clone()
                route = (C.c_int * n)()
                _lib.check(L.ipk_pipeline_batch_each_plan(dp, n, 1, route, None), "ipk_pipeline_batch_each_plan")
                assert list(route) == [2] * n, (name, n, list(route))
                out.zero_()
                with ipa.launch_log() as ran:
                    run(); torch.cuda.synchronize()
                assert len([e for e in ran if "k_raw_scaled_demosaic<unsigned short>[" in e and "frames=1,sized=1]" in e]) == 1, (name, n, sorted(ran))
                assert len([e for e in ran if "k_raster_chain<" in e and "sized=1]" in e]) >= 1, (name, n, sorted(ran))
                assert torch.equal(out, want), "%s, n = %d: the new call differs from this build's loop" % (name, n)
                res["sized"] = _wall(run, runs)
                for key, pick in (("first", lambda i: 0), ("second", lambda i: 1)):
                    d2, s2, p2 = build(pick)
                    for d in d2:
                        d.allow_fused = OLD_BITS | SIZES
                    out2 = torch.zeros(sum(s[2] for s in s2[:n]), dtype=torch.uint8, device="cuda")
                    _, run2 = each(d2, s2, p2, n, out2)
                    with ipa.launch_log() as ran:
                        run2(); torch.cuda.synchronize()
                    assert not [e for e in ran if "sized=1" in e], sorted(ran)
                    res[key] = _wall(run2, runs)
            print("RESULT " + json.dumps(res), flush=True)
        del frames
        torch.cuda.empty_cache()


def summarise(acc, rounds, runs):
    import numpy as np
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["batch_sizes_probe: noise frames, device-resident sources, 8-bit outputs into one allocation, every frame with its own wb_coeffs; %d rounds of" % rounds,
             "(parent, new) as alternating child processes on one box; wall clock around the call and a synchronise, ms PER FRAME (the time / n), medians with the",
             "fastest run in brackets; %d runs per round, 3 warm-ups; spread = the parent's p95 - median, per frame.  parent = the parent build's" % runs,
             "ipk_pipeline_run_batch_each, which cuts the run at every frame (a loop of ipk_pipeline_run, two launches per frame); sized = this build's call with",
             "IPK_FUSED_BATCH_SIZES (route 2: ONE sized scaling launch and ONE sized point-wise launch per chunk); first / second = this build's route 2 on frames",
             "that all have the first / second shape (equal sizes, the launches of bits 9 and 10): sized - mean(first, second) is the price of the spread of sizes", ""]
    slower, outside, gains, waste = [], [], {}, {}
    for name, shapes, mw in CASES:
        first = True
        for n in NS:
            c = acc.get((name, n))
            if c is None or ("new", "sized") not in c["t"] or ("parent", "parent") not in c["t"]:
                lines.append("  %s, n = %d: not measured" % (name, n))
                continue
            if first:
                lines.append("  %s (demosaic %s)" % (name, c.get("demosaic")))
                first = False
            P, S = ([v / n for v in c["t"][k]] for k in (("parent", "parent"), ("new", "sized")))
            if n >= 8 and med(S) > med(P):
                slower.append("%s at n = %d (sized %.4f ms per frame, parent %.4f, spread %.4f)" % (name, n, med(S), med(P), spread(P)))
            gains.setdefault(n, []).append(med(P) / med(S))
            eq = ""
            if ("new", "first") in c["t"] and ("new", "second") in c["t"]:
                A, B = ([v / n for v in c["t"][("new", k)]] for k in ("first", "second"))
                waste.setdefault(n, []).append(med(S) - 0.5 * (med(A) + med(B)))
                eq = "  first %7.4f  second %7.4f   %+.4f ms for the spread" % (med(A), med(B), med(S) - 0.5 * (med(A) + med(B)))
            lines.append("    n = %2d   parent %7.4f (%.4f; spread %.4f)  sized %7.4f (%.4f)   x%.2f over the parent%s"
                         % (n, med(P), low(P), spread(P), med(S), low(S), med(P) / med(S), eq))
    lines += ["", "launches outside the mode, parent -> this build (ms per call, medians with the fastest run in brackets):"]
    for name in UNTOUCHED:
        c = acc.get((name, -1))
        if c is None or ("new", "single") not in c["t"] or ("parent", "single") not in c["t"]:
            lines.append("    %-72s not measured" % name)
            continue
        P, N = c["t"][("parent", "single")], c["t"][("new", "single")]
        inside = abs(med(N) - med(P)) <= spread(P)
        if not inside:
            outside.append("%s (%.4f -> %.4f ms, spread %.4f)" % (name, med(P), med(N), spread(P)))
        lines.append("    %-72s %7.4f (%.4f; spread %.4f) -> %7.4f (%.4f)   %s"
                     % (name, med(P), low(P), spread(P), med(N), low(N), "inside the parent's spread" if inside else
                        ("FASTER than the parent beyond its spread" if med(N) < med(P) else "SLOWER than the parent beyond its spread")))
    lines += ["", "sized over the parent's loop, per frame, smallest .. largest over the cases: " +
              "; ".join("n = %d: x%.2f .. x%.2f" % (n, min(v), max(v)) for n, v in sorted(gains.items())),
              "sized minus the mean of the two equal-size runs, ms per frame, smallest .. largest over the cases (wasted blocks, the larger records; reported, not bounded): " +
              "; ".join("n = %d: %+.4f .. %+.4f" % (n, min(v), max(v)) for n, v in sorted(waste.items())),
              "launches outside the mode that left the parent's spread: " + ("none" if not outside else "; ".join(outside)),
              "cases at n >= 8 where the sized route is SLOWER than the parent's loop: " + ("none" if not slower else "; ".join(slower)),
              "not measured: f32 sources, f32 and 16-bit outputs, mosaics other than RGGB, monochrome and three-sample raws, more than two sizes in a chunk, batches",
              "above 64 frames, chunks cut by the 256 MiB sum, orientation and sensor size together, the host cost of the plan alone, photo-like data"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_batch_sizes.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"])
    ap.add_argument("--untouched-only", action="store_true", help="only the launches outside the mode")
    ap.add_argument("--limit", type=int, default=300, help="seconds a worker may take")
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new", a.untouched_only)
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline")
    builds = [("parent", os.path.abspath(a.parent)), ("new", None)]
    acc = {}
    for rnd in range(a.rounds):
        for label, so in builds:
            env = dict(os.environ)
            env.pop("IPK_SO_OVERRIDE", None)
            if so:
                env["IPK_SO_OVERRIDE"] = so
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", label, "--runs", str(a.runs)]
            if a.untouched_only:
                cmd.append("--untouched-only")
            p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            seen = []
            for line in p.stdout:
                seen.append(line)
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    print("  round %d %s: %s, n = %d" % (rnd, label, r["case"], r["n"]), flush=True)
            if p.wait() != 0:
                sys.stderr.write("".join(seen))
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (label, p.returncode))
            for line in seen:
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault((r["case"], r["n"]), dict(t={}))
                    for k, v in r.items():
                        if isinstance(v, list):
                            c["t"].setdefault((label, k), []).extend(v)
                        elif k not in ("case", "n"):
                            c[k] = v
            print("round %d %s done" % (rnd, label), flush=True)
    lines = summarise(acc, a.rounds, a.runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
