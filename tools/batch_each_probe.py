#!/usr/bin/env python
"""Development tool: what a shoot of thumbnails costs per frame when every file carries its own white balance and exposure.  The PARENT build offers such a
caller one thing: a loop of ipk_pipeline_run over the per-frame descriptors, two launches per frame.  This build's ipk_pipeline_run_batch_each runs the
frames as varied previews (route 2 of ipk_pipeline_batch_each_plan): the shared scaling launch and ONE point-wise launch per chunk, whose per-frame
parameters come from a table on the device.  Columns: the parent's loop; this build's new call with IPK_FUSED_BATCH_PREVIEWS clear (its loop); the new call
with the bit set; this build's uniform ipk_pipeline_run_batch on ONE descriptor as the yardstick (what the table upload and the per-frame staging cost).
Also the launches of the carrier kernels that do not use the mode, in both builds: single-frame ipk_pointwise_chain_out at 2160x1440 and 6000x4000 to f32
and to u8, and the cached-region gather launch over 1/16 of a 24 MP frame.

Frames (noise, device-resident, 8-bit outputs into one allocation): 24 MP RGGB u16 -> 256 and 400 wide, 50 MP X-Trans u16 -> 270 wide, 24 MP mono u16 ->
256 wide, each at n = 2, 8, 16, 64.  Before anything is timed the new call with the bit is compared with this build's loop (all frames, equal bytes) and,
in the first round, frame n - 1 of the smallest batch with the CPU oracle on that frame's own settings; the plan must say route 2, the launch log must
show the carrier with batch=1 and ipk_timing two stages per chunk.  Wall clock around the call and a stream synchronise, 3 warm-ups, medians and minima
over all rounds; the parent build and this build alternate as child processes of one session on one box; spread = the parent's p95 - median.
usage: tools/batch_each_probe.py --parent /path/to/libparent.so [--out profiles/r20_batch_each.txt]"""
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
# name, kind, width, height, maxwidth
CASES = [("24 MP RGGB u16 -> 256 wide", "RGGB", 6000, 4000, 256), ("24 MP RGGB u16 -> 400 wide", "RGGB", 6000, 4000, 400),
         ("50 MP X-Trans u16 -> 270 wide", XT, 8640, 5760, 270), ("24 MP mono u16 -> 256 wide", "mono", 6000, 4000, 256)]
NS = [2, 8, 16, 64]
OLD_BITS = 255                                                            # every bit below IPK_FUSED_BATCH_PREVIEWS
BATCH = 256
CHAINS = [("chain 2160x1440 -> f32", 2160, 1440, 0), ("chain 2160x1440 -> u8", 2160, 1440, 1), ("chain 6000x4000 -> f32", 6000, 4000, 0),
          ("chain 6000x4000 -> u8", 6000, 4000, 1)]
GATHER = "cached-region gather, 1/16 of 24 MP -> u8"


def _wall(run, runs, warm=3):
    import torch
    ts = []
    for k in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); run(); torch.cuda.synchronize()
        if k >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def _settings(util, i):
    """frame i's own white balance and exposure"""
    return (util.WB[0] * (1.0 + i / 128.0), util.WB[1], util.WB[2] * (1.0 - i / 256.0), util.WB[3]), (i % 9 - 4) / 16.0


def _pipe(ipa, util, kind, w, h, mw, data):
    pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=data, cfa="" if kind == "mono" else kind, cpp=1, blacklevels=[util.BLACK] * 4,
                                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    pipe.globals.settings.maxwidth = mw
    return pipe


def _oracle(util, frame, kind, w, h, mw, wb, exposure):
    import numpy as np
    import oracle as orc
    host = frame.cpu().numpy().view(np.uint16).reshape(h, w)
    desc = orc.make_pipeline(host, cfa="" if kind == "mono" else kind, cpp=1, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=wb,
                             exposure=exposure, cam_to_xyz_normalized=util.cam_matrix(), maxwidth=mw)
    return orc.pipeline_output_8bit(desc)


def untouched(runs, ipa, util, L, _lib):
    """the carriers' launches outside the mode"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    wb = (C.c_float * 4)(*util.WB)
    cm = (C.c_float * 12)(*[float(v) for v in util.cam_matrix().ravel()])
    pts = (C.c_float * 2)(0.5, 0.6)
    for name, w, h, out in CHAINS:
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 200)
        src = torch.rand((w * h, 4), device="cuda", generator=g, dtype=torch.float32)
        src[:, 3] = 0.0
        dst = torch.empty(w * h * 3, dtype=torch.float32 if out == 0 else torch.uint8, device="cuda")
        run = lambda: _lib.check(L.ipk_pointwise_chain_out(src.data_ptr(), w, h, 0, wb, cm, 0.0, pts, 1, 0, out, dst.data_ptr(), st), "ipk_pointwise_chain_out")
        with ipa.launch_log() as ran:
            run(); torch.cuda.synchronize()
        assert len(ran) == 1 and "batch" not in list(ran)[0], sorted(ran)
        print("RESULT " + json.dumps({"case": name, "n": -1, "kernel": list(ran)[0].split("[")[0], "single": _wall(run, 2 * runs)}), flush=True)
        del src, dst
    w, h = 6000, 4000
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 201)
    frame = torch.randint(0, 16384, (w * h,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    pipe = _pipe(ipa, util, "RGGB", w, h, 0, frame)
    cache = ipa.PipelineCache(6 << 30)
    full = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
    pipe._run(1, out=full, cache=cache)
    pipe.ops.basecurve.exposure = 0.05
    cache.clear()
    pipe.allow_fused = False; pipe._run(1, out=full, cache=cache); pipe.allow_fused = True     # a staged run fills the cache up to OpRotateCrop
    reg = torch.empty(1500 * 1000 * 3, dtype=torch.uint8, device="cuda")
    step = [0]

    def run():
        step[0] += 1
        pipe.ops.basecurve.exposure = 0.05 + 0.01 * (step[0] % 7)
        pipe.run_region(2000, 1500, 1500, 1000, 1, out=reg, cache=cache)
    with ipa.launch_log() as ran:
        run(); torch.cuda.synchronize()
    hits = [e for e in ran if "gather=1" in e]
    if hits:                                                              # (no such launch: the line is left out of the report, which says so)
        print("RESULT " + json.dumps({"case": GATHER, "n": -1, "kernel": hits[0].split("[")[0], "single": _wall(run, 2 * runs)}), flush=True)
    cache.close()


def worker(runs, new_build, oracle):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case and batch size"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    import util
    ipa.init(0)
    L = ipa.lib()
    untouched(runs, ipa, util, L, _lib)
    for ci, (name, kind, w, h, mw) in enumerate(CASES):
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 210 + ci)
        frames = [torch.randint(0, 16384, (w * h,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16) for _ in range(max(NS))]
        pipe = _pipe(ipa, util, kind, w, h, mw, frames[0])
        (dw, dh), (fw, fh) = pipe.sizes()
        px3 = fw * fh * 3
        st = torch.cuda.current_stream().cuda_stream
        descs = []
        for i in range(max(NS)):
            d = _lib.PipelineDesc.from_buffer_copy(pipe.desc())
            wb, exposure = _settings(util, i)
            d.wb_coeffs[:] = wb
            d.exposure = exposure
            descs.append(d)

        def set_mask(mask):
            for d in descs:
                d.allow_fused = mask

        def loop(n, out):                                                 # the parent's only offer: ipk_pipeline_run per frame
            def run():
                for i in range(n):
                    _lib.check(L.ipk_pipeline_run(C.byref(descs[i]), frames[i].data_ptr(), out.data_ptr() + i * px3, 1, None, st), "ipk_pipeline_run")
            return run

        def each(n, out):
            dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
            sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
            op = (C.c_void_p * n)(*[out.data_ptr() + i * px3 for i in range(n)])
            return lambda: _lib.check(L.ipk_pipeline_run_batch_each(dp, sp, op, n, 1, None, st), "ipk_pipeline_run_batch_each")

        def uniform(n, out):
            sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
            op = (C.c_void_p * n)(*[out.data_ptr() + i * px3 for i in range(n)])
            return lambda: _lib.check(L.ipk_pipeline_run_batch(C.byref(descs[0]), sp, op, n, 1, None, st), "ipk_pipeline_run_batch")
        for n in NS:
            res = dict(case=name, n=n, demosaic="%dx%d" % (dw, dh))
            out = torch.zeros(n * px3, dtype=torch.uint8, device="cuda")
            set_mask(OLD_BITS)
            loop(n, out)(); torch.cuda.synchronize()
            want = out.clone()
            if new_build:
                set_mask(OLD_BITS | BATCH)
                dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
                route = (C.c_int * n)()
                _lib.check(L.ipk_pipeline_batch_each_plan(dp, n, 1, route, None), "ipk_pipeline_batch_each_plan")
                assert list(route) == [2] * n, (name, n, list(route))
                out.zero_()
                run = each(n, out)
                _lib.check(L.ipk_timing_begin(), "ipk_timing_begin")
                with ipa.launch_log() as ran:
                    run(); torch.cuda.synchronize()
                arr = (_lib.StageTime * 8)(); ns = C.c_int(0)
                _lib.check(L.ipk_timing_end(arr, 8, C.byref(ns)), "ipk_timing_end")
                assert ns.value == 2 and len([e for e in ran if "k_raster_chain<ipk::Rgbe32, 1>[" in e and "batch=1" in e]) == 1, (name, n, ns.value, sorted(ran))
                assert torch.equal(out, want), "%s, n = %d: the new call differs from this build's loop" % (name, n)
                if oracle and n == NS[0]:
                    i = n - 1
                    wb, exposure = _settings(util, i)
                    assert np.array_equal(out[i * px3: (i + 1) * px3].cpu().numpy().reshape(fh, fw, 3), _oracle(util, frames[i], kind, w, h, mw, wb, exposure)), \
                        "%s: frame %d differs from the oracle's" % (name, i)
                    res["oracle"] = 1
                res["each"] = _wall(run, runs)
                res["uniform"] = _wall(uniform(n, out), runs)
                set_mask(OLD_BITS)
                res["each_off"] = _wall(each(n, out), runs)
            set_mask(OLD_BITS)
            res["loop"] = _wall(loop(n, out), runs)
            print("RESULT " + json.dumps(res), flush=True)
        del frames, pipe
        torch.cuda.empty_cache()


def summarise(acc, rounds, runs):
    """acc: {(case, n): {"demosaic": ..., "oracle": ..., "t": {(build, key): [ms, ...]}}} -> the report's lines"""
    import numpy as np
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["batch_each_probe: noise frames, device-resident sources, 8-bit outputs into one allocation, every frame with its own wb_coeffs and exposure; %d rounds" % rounds,
             "of (parent, new) as alternating child processes on one box; wall clock around the call(s) and a synchronise, ms PER FRAME (the time / n), medians with",
             "the fastest run in brackets; %d runs per round, 3 warm-ups; spread = the parent's p95 - median, per frame.  parent = the parent build's only offer, a loop" % runs,
             "of ipk_pipeline_run over the per-frame descriptors (two launches per frame; every bit it knows set); off = this build's ipk_pipeline_run_batch_each with",
             "IPK_FUSED_BATCH_PREVIEWS clear; each = the same call with the bit set (route 2: the shared scaling launch and ONE point-wise launch per 64 frames, the",
             "per-frame parameters from a device table); uniform = this build's ipk_pipeline_run_batch on ONE descriptor, the yardstick.", ""]
    slower, outside, gains, dist = [], [], {}, {}
    for name, kind, w, h, mw in CASES:
        first = True
        for n in NS:
            c = acc.get((name, n))
            if c is None or ("new", "each") not in c["t"]:
                continue
            if first:
                lines.append("  %s (demosaic %s)" % (name, c.get("demosaic")))
                first = False
            P, O, E, U = ([v / n for v in c["t"][(b, k)]] for b, k in (("parent", "loop"), ("new", "each_off"), ("new", "each"), ("new", "uniform")))
            if n >= 8 and med(E) > med(P) + spread(P):
                slower.append("%s at n = %d (each %.4f ms per frame, parent %.4f, spread %.4f)" % (name, n, med(E), med(P), spread(P)))
            gains.setdefault(n, []).append(med(P) / med(E))
            dist.setdefault(n, []).append(med(E) - med(U))
            lines.append("    n = %2d   parent %7.4f (%.4f; spread %.4f)  off %7.4f (%.4f)  each %7.4f (%.4f)  uniform %7.4f (%.4f)   x%.2f over the parent, %+.4f ms to the uniform batch%s"
                         % (n, med(P), low(P), spread(P), med(O), low(O), med(E), low(E), med(U), low(U), med(P) / med(E), med(E) - med(U),
                            "; checked against the oracle" if c.get("oracle") else ""))
    lines += ["", "launches of the carrier kernels outside the mode, parent -> this build (ms, medians with the fastest run in brackets):"]
    for name in [c[0] for c in CHAINS] + [GATHER]:
        c = acc.get((name, -1))
        if c is None or ("new", "single") not in c["t"] or ("parent", "single") not in c["t"]:
            lines.append("    %-44s not measured (the launch did not occur)" % name)
            continue
        P, N = c["t"][("parent", "single")], c["t"][("new", "single")]
        inside = abs(med(N) - med(P)) <= spread(P)
        if not inside:
            outside.append("%s (%.4f -> %.4f ms, spread %.4f)" % (name, med(P), med(N), spread(P)))
        lines.append("    %-44s %-40s %7.4f (%.4f; spread %.4f) -> %7.4f (%.4f)   %s"
                     % (name, c.get("kernel", "").replace("ipk::", ""), med(P), low(P), spread(P), med(N), low(N), "inside the parent's spread" if inside else
                        ("FASTER than the parent beyond its spread" if med(N) < med(P) else "SLOWER than the parent beyond its spread")))
    lines += ["", "each over the parent's loop, per frame, smallest .. largest over the cases: " +
              "; ".join("n = %d: x%.2f .. x%.2f" % (n, min(v), max(v)) for n, v in sorted(gains.items())),
              "each minus the uniform batch, ms per frame, smallest .. largest over the cases (the table upload and the per-frame staging; reported, not bounded): " +
              "; ".join("n = %d: %+.4f .. %+.4f" % (n, min(v), max(v)) for n, v in sorted(dist.items())),
              "untouched launches outside the parent's spread: " + ("none" if not outside else "; ".join(outside)),
              "cases at n >= 8 where the varied route is SLOWER than the parent's loop beyond the parent's spread: " + ("none" if not slower else "; ".join(slower)),
              "not measured: f32 sources, f32 and 16-bit outputs, scattered destinations, per-frame matrices and curves (the table record is the same size whatever",
              "differs), batches above 64 frames, rasters and the window-8 geometries (pass 1 per frame), mixed batches, the host cost of the plan alone, photo-like data"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_batch_each.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"]); ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--limit", type=int, default=400, help="seconds a worker may take")
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker == "new", a.oracle)
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
            if rnd == 0 and label == "new":
                cmd.append("--oracle")
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
