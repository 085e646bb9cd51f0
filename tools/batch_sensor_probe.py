#!/usr/bin/env python
"""Development tool: what a shoot of thumbnails costs per frame when every file carries its own SENSOR settings -- black and white levels that move with
the ISO, or two bodies with different sensor sizes.  The PARENT build offers such a caller one thing: its ipk_pipeline_run_batch_each cuts the run at
every such frame, a loop of ipk_pipeline_run, two launches per frame.  This build's call with IPK_FUSED_BATCH_SENSOR keeps the frames in one varied run:
ONE frame-table scaling launch and ONE point-wise launch per 64 frames.  Columns: parent = the parent build's ipk_pipeline_run_batch_each on the same
descriptors (every bit it knows set); sensor = this build's call with the bit; equal = this build's route 2 on the same frames with EQUAL sensor fields
(colours varied alone: the uniform scaling launch), the price of the table.  One series alternates two sensor sizes.  Also the carrier kernel's untouched
modes in both builds: ipk_raw_scaled_demosaic on a general-kernel geometry and ipk_raw_scaled_demosaic_batch at n = 8 and 64.

Frames (noise, device-resident, 8-bit outputs into one allocation): 24 MP RGGB u16 -> 256 and 400 wide, 50 MP X-Trans u16 -> 270 wide, 24 MP mono u16 ->
256 wide, 24 MP + 24.4 MP RGGB alternating -> 256 wide, each at n = 2, 8, 16, 64.  Before anything is timed the new call is compared with this build's
loop of ipk_pipeline_run (all frames, equal bytes); the plan must say route 2 and the launch log must show the frame-table launch (frames=1).  Wall clock
around the call and a stream synchronise, 3 warm-ups, medians and minima over all rounds; the parent build and this build alternate as child processes of
one session on one box; spread = the parent's p95 - median.
usage: tools/batch_sensor_probe.py --parent /path/to/libparent.so [--out profiles/r22_batch_sensor.txt]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
# name, kind, [(width, height), ...] (frame i takes entry i mod len), maxwidth
CASES = [("24 MP RGGB u16 -> 256 wide", "RGGB", [(6000, 4000)], 256), ("24 MP RGGB u16 -> 400 wide", "RGGB", [(6000, 4000)], 400),
         ("50 MP X-Trans u16 -> 270 wide", XT, [(8640, 5760)], 270), ("24 MP mono u16 -> 256 wide", "mono", [(6000, 4000)], 256),
         ("24 MP / 24.4 MP RGGB u16 alternating -> 256 wide", "RGGB", [(6000, 4000), (6048, 4032)], 256)]
NS = [2, 8, 16, 64]
OLD_BITS = 255 | 256 | 512                                                # every bit the parent knows
SENSOR = 1024
SINGLE = "ipk_raw_scaled_demosaic 6000x4000 -> 400x266"
BATCHES = [("ipk_raw_scaled_demosaic_batch 6000x4000 -> 256x170, n = 8", 8), ("ipk_raw_scaled_demosaic_batch 6000x4000 -> 256x170, n = 64", 64)]


def _wall(run, runs, warm=3):
    import torch
    ts = []
    for k in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); run(); torch.cuda.synchronize()
        if k >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def _levels(util, i):
    """frame i's own levels"""
    return util.BLACK + float(i % 7), util.WHITE - 3.0 * (i % 5)


def _wb(util, i):
    return (util.WB[0] * (1.0 + i / 128.0), util.WB[1], util.WB[2] * (1.0 - i / 256.0), util.WB[3])


def _pipe(ipa, util, kind, w, h, mw, data):
    pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=data, cfa="" if kind == "mono" else kind, cpp=1, blacklevels=[util.BLACK] * 4,
                                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    pipe.globals.settings.maxwidth = mw
    return pipe


def untouched(runs, ipa, util, L, _lib, frames):
    """the carrier kernel's launches outside the mode: the single launch and the uniform batch launch"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    w, h = 6000, 4000
    dst = torch.empty(64 * 256 * 170 * 4 + 400 * 266 * 4, dtype=torch.float32, device="cuda")
    run = lambda: _lib.check(L.ipk_raw_scaled_demosaic(frames[0].data_ptr(), 0, w, 0, 0, w, h, util.BLACK, util.WHITE, b"RGGB", 400, 266, dst.data_ptr(), st),
                             "ipk_raw_scaled_demosaic")
    with ipa.launch_log() as ran:
        run(); torch.cuda.synchronize()
    assert len(ran) == 1 and "k_raw_scaled_demosaic<unsigned short>[" in list(ran)[0] and "batch" not in list(ran)[0], sorted(ran)
    print("RESULT " + json.dumps({"case": SINGLE, "n": -1, "single": _wall(run, 2 * runs)}), flush=True)
    for name, n in BATCHES:
        sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
        run = lambda: _lib.check(L.ipk_raw_scaled_demosaic_batch(sp, n, 0, w, 0, 0, w, h, util.BLACK, util.WHITE, b"RGGB", 256, 170, dst.data_ptr(), st),
                                 "ipk_raw_scaled_demosaic_batch")
        with ipa.launch_log() as ran:
            run(); torch.cuda.synchronize()
        assert len(ran) == 1 and list(ran)[0].endswith("xcd=0,batch=1]"), sorted(ran)
        print("RESULT " + json.dumps({"case": name, "n": -1, "single": _wall(run, 2 * runs)}), flush=True)


def worker(runs, new_build, untouched_only=False):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case and batch size"""
    import torch
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    import util
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    for ci, (name, kind, shapes, mw) in enumerate(CASES):
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 220 + ci)
        dims = [shapes[i % len(shapes)] for i in range(max(NS))]
        frames = [torch.randint(0, 16384, (w * h,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16) for w, h in dims]
        if ci == 0:
            untouched(runs, ipa, util, L, _lib, frames)
            if untouched_only:
                return
        descs, px3, demosaic = [], None, None
        for i, (w, h) in enumerate(dims):
            pipe = _pipe(ipa, util, kind, w, h, mw, frames[i])
            (dw, dh), (fw, fh) = pipe.sizes()
            assert demosaic in (None, (dw, dh)), (name, demosaic, (dw, dh))
            demosaic, px3 = (dw, dh), fw * fh * 3
            d = _lib.PipelineDesc.from_buffer_copy(pipe.desc())
            d.wb_coeffs[:] = _wb(util, i)
            descs.append(d)

        def settle(mask, own_levels):
            for i, d in enumerate(descs):
                d.allow_fused = mask
                b, w = _levels(util, i) if own_levels else (util.BLACK, util.WHITE)
                d.blacklevels[:] = [b] * 4
                d.whitelevels[:] = [w] * 4

        def loop(n, out):
            def run():
                for i in range(n):
                    _lib.check(L.ipk_pipeline_run(C.byref(descs[i]), frames[i].data_ptr(), out.data_ptr() + i * px3, 1, None, st), "ipk_pipeline_run")
            return run

        def each(n, out):
            dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
            sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
            op = (C.c_void_p * n)(*[out.data_ptr() + i * px3 for i in range(n)])
            return lambda: _lib.check(L.ipk_pipeline_run_batch_each(dp, sp, op, n, 1, None, st), "ipk_pipeline_run_batch_each")
        for n in NS:
            res = dict(case=name, n=n, demosaic="%dx%d" % demosaic)
            out = torch.zeros(n * px3, dtype=torch.uint8, device="cuda")
            if not new_build:
                settle(OLD_BITS, True)
                res["parent"] = _wall(each(n, out), runs)
            else:
                settle(OLD_BITS | SENSOR, True)
                loop(n, out)(); torch.cuda.synchronize()
                want = out.clone()
                dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
                route = (C.c_int * n)()
                _lib.check(L.ipk_pipeline_batch_each_plan(dp, n, 1, route, None), "ipk_pipeline_batch_each_plan")
                assert list(route) == [2] * n, (name, n, list(route))
                out.zero_()
                run = each(n, out)
                with ipa.launch_log() as ran:
                    run(); torch.cuda.synchronize()
                assert len([e for e in ran if "k_raw_scaled_demosaic<unsigned short>[" in e and "batch=1,frames=1]" in e]) == 1, (name, n, sorted(ran))
                assert torch.equal(out, want), "%s, n = %d: the new call differs from this build's loop" % (name, n)
                res["sensor"] = _wall(run, runs)
                if len(shapes) == 1:
                    settle(OLD_BITS | SENSOR, False)
                    run = each(n, out)
                    with ipa.launch_log() as ran:
                        run(); torch.cuda.synchronize()
                    assert not [e for e in ran if "frames=1" in e] and [e for e in ran if e.endswith("batch=1]") and "k_raw_scaled_demosaic<" in e], sorted(ran)
                    res["equal"] = _wall(run, runs)
            print("RESULT " + json.dumps(res), flush=True)
        del frames
        torch.cuda.empty_cache()


def summarise(acc, rounds, runs):
    import numpy as np
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["batch_sensor_probe: noise frames, device-resident sources, 8-bit outputs into one allocation, every frame with its own black and white level and its",
             "own wb_coeffs; %d rounds of (parent, new) as alternating child processes on one box; wall clock around the call and a synchronise, ms PER FRAME (the" % rounds,
             "time / n), medians with the fastest run in brackets; %d runs per round, 3 warm-ups; spread = the parent's p95 - median, per frame.  parent = the parent" % runs,
             "build's ipk_pipeline_run_batch_each, which cuts the run at every frame (a loop of ipk_pipeline_run, two launches per frame); sensor = this build's call",
             "with IPK_FUSED_BATCH_SENSOR (route 2: ONE frame-table scaling launch and ONE point-wise launch per 64 frames); equal = this build's route 2 on the same",
             "frames with equal levels (the uniform scaling launch): sensor - equal is the price of the table.", ""]
    slower, outside, gains, price = [], [], {}, {}
    for name, kind, shapes, mw in CASES:
        first = True
        for n in NS:
            c = acc.get((name, n))
            if c is None or ("new", "sensor") not in c["t"] or ("parent", "parent") not in c["t"]:
                continue
            if first:
                lines.append("  %s (demosaic %s)" % (name, c.get("demosaic")))
                first = False
            P, S = ([v / n for v in c["t"][k]] for k in (("parent", "parent"), ("new", "sensor")))
            E = [v / n for v in c["t"][("new", "equal")]] if ("new", "equal") in c["t"] else None
            if n >= 8 and med(S) > med(P) + spread(P):
                slower.append("%s at n = %d (sensor %.4f ms per frame, parent %.4f, spread %.4f)" % (name, n, med(S), med(P), spread(P)))
            gains.setdefault(n, []).append(med(P) / med(S))
            eq = "  equal       --       "
            if E is not None:
                price.setdefault(n, []).append(med(S) - med(E))
                eq = "  equal %7.4f (%.4f)   %+.4f ms for the table" % (med(E), low(E), med(S) - med(E))
            lines.append("    n = %2d   parent %7.4f (%.4f; spread %.4f)  sensor %7.4f (%.4f)   x%.2f over the parent%s"
                         % (n, med(P), low(P), spread(P), med(S), low(S), med(P) / med(S), eq))
    lines += ["", "the carrier kernel's untouched modes, parent -> this build (ms per call, medians with the fastest run in brackets):"]
    for name in [SINGLE] + [b[0] for b in BATCHES]:
        c = acc.get((name, -1))
        if c is None or ("new", "single") not in c["t"] or ("parent", "single") not in c["t"]:
            lines.append("    %-64s not measured" % name)
            continue
        P, N = c["t"][("parent", "single")], c["t"][("new", "single")]
        inside = abs(med(N) - med(P)) <= spread(P)
        if not inside:
            outside.append("%s (%.4f -> %.4f ms, spread %.4f)" % (name, med(P), med(N), spread(P)))
        lines.append("    %-64s %7.4f (%.4f; spread %.4f) -> %7.4f (%.4f)   %s"
                     % (name, med(P), low(P), spread(P), med(N), low(N), "inside the parent's spread" if inside else
                        ("FASTER than the parent beyond its spread" if med(N) < med(P) else "SLOWER than the parent beyond its spread")))
    lines += ["", "sensor over the parent's loop, per frame, smallest .. largest over the cases: " +
              "; ".join("n = %d: x%.2f .. x%.2f" % (n, min(v), max(v)) for n, v in sorted(gains.items())),
              "sensor minus equal, ms per frame, smallest .. largest over the cases (the record upload, per-frame negotiation and scalar loads; reported, not bounded): " +
              "; ".join("n = %d: %+.4f .. %+.4f" % (n, min(v), max(v)) for n, v in sorted(price.items())),
              "untouched modes outside the parent's spread: " + ("none" if not outside else "; ".join(outside)),
              "cases at n >= 8 where the sensor route is SLOWER than the parent's loop beyond the parent's spread: " + ("none" if not slower else "; ".join(slower)),
              "not measured: f32 sources, f32 and 16-bit outputs, per-frame crops and filters inside one series (the record is the same size whatever differs),",
              "three-sample raws, batches above 64 frames, orientations beside sensor settings, mixed batches, the host cost of the plan alone, photo-like data"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_batch_sensor.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"])
    ap.add_argument("--untouched-only", action="store_true", help="only the carrier kernel's untouched modes (a closer look at them: more rounds, more runs)")
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
            # the worker's lines are read as they come, so that a long case still shows progress
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
