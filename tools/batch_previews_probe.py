#!/usr/bin/env python
"""Development tool: what a batch of thumbnails costs per frame under IPK_FUSED_BATCH_PREVIEWS -- the scaling pass of up to 64 frames as ONE launch of
k_raw_scaled_demosaic<T>'s batch mode, then the point-wise chain ONCE over the previews lying one after another -- against the PARENT build's
ipk_pipeline_run_batch of the same descriptor (its loop: a scaling launch and a chain launch per frame; every bit the parent knows set), and against this
build's own loop (the bit clear).  Also the single-frame general kernel (ipk_raw_scaled_demosaic / ipk_plain_scale_down, same geometries) in both builds:
what the added kernel argument and the frame select cost a launch that uses neither.

Frames (noise, device-resident, 8-bit outputs into one allocation): 24 MP RGGB u16 -> 256 and 400 wide, 50 MP X-Trans u16 -> 270 wide, 24 MP mono u16 ->
256 wide, each at n = 2, 8, 16, 64.  Before anything is timed the batch with the bit is compared with this build's loop (all frames, equal bytes) and, in
the first round, frames 0 and n - 1 of the smallest batch with the CPU oracle; the launch log must show batch=1 and ipk_timing two stages per chunk.
Wall clock around the call and a stream synchronise, 3 warm-ups, medians and minima over all rounds; the parent build and this build alternate as child
processes of one session on one box; spread = the parent's p95 - median.  HBM floor: the source's bytes per frame at 6.3 TB/s (tools/copy_probe.hip).
usage: tools/batch_previews_probe.py --parent /path/to/libparent.so [--out profiles/r19_batch_previews.txt]"""
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
OLD_BITS = 255                                                            # every bit the parent knows
BATCH = 256
HBM_TBS = 6.3


def _wall(run, runs, warm=3):
    import torch
    ts = []
    for k in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); run(); torch.cuda.synchronize()
        if k >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def _pipe(ipa, util, kind, w, h, mw, data):
    pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=data, cfa="" if kind == "mono" else kind, cpp=1, blacklevels=[util.BLACK] * 4,
                                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    pipe.globals.settings.maxwidth = mw
    return pipe


def _oracle(util, frame, kind, w, h, mw):
    import numpy as np
    import oracle as orc
    host = frame.cpu().numpy().view(np.uint16).reshape(h, w)
    desc = orc.make_pipeline(host, cfa="" if kind == "mono" else kind, cpp=1, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                             cam_to_xyz_normalized=util.cam_matrix(), maxwidth=mw)
    return orc.pipeline_output_8bit(desc)


def worker(runs, new_build, oracle):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case and batch size"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    import util
    ipa.init(0)
    L = ipa.lib()
    for ci, (name, kind, w, h, mw) in enumerate(CASES):
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 190 + ci)
        frames = [torch.randint(0, 16384, (w * h,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16) for _ in range(max(NS))]
        pipe = _pipe(ipa, util, kind, w, h, mw, frames[0])
        d = pipe.desc()
        (dw, dh), (fw, fh) = pipe.sizes()
        px3 = fw * fh * 3
        st = torch.cuda.current_stream().cuda_stream

        def batch(mask, n, out):
            sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
            dp = (C.c_void_p * n)(*[out.data_ptr() + i * px3 for i in range(n)])

            def run():
                d.allow_fused = mask
                _lib.check(L.ipk_pipeline_run_batch(C.byref(d), sp, dp, n, 1, None, st), "ipk_pipeline_run_batch")
            return run
        # the single-frame general kernel, same geometry
        rgbe = torch.empty(dw * dh * 4, dtype=torch.float32, device="cuda")
        lv = (C.c_float * 4)(*[util.BLACK] * 4), (C.c_float * 4)(*[util.WHITE] * 4)
        if kind == "mono":
            one = lambda: _lib.check(L.ipk_plain_scale_down(frames[0].data_ptr(), 0, 2, w, 0, 0, w, h, lv[0], lv[1], dw, dh, rgbe.data_ptr(), st), "ipk_plain_scale_down")
        else:
            one = lambda: _lib.check(L.ipk_raw_scaled_demosaic(frames[0].data_ptr(), 0, w, 0, 0, w, h, util.BLACK, util.WHITE, kind.encode(), dw, dh, rgbe.data_ptr(), st),
                                     "ipk_raw_scaled_demosaic")
        with ipa.launch_log() as ran:
            one(); torch.cuda.synchronize()
        assert len(ran) == 1 and "k_raw_scaled_demosaic<unsigned short>[" in list(ran)[0] and "batch" not in list(ran)[0], sorted(ran)
        print("RESULT " + json.dumps({"case": name, "n": 0, "demosaic": "%dx%d" % (dw, dh), "single": _wall(one, 2 * runs)}), flush=True)
        for n in NS:
            res = dict(case=name, n=n, demosaic="%dx%d" % (dw, dh))
            out = torch.zeros(n * px3, dtype=torch.uint8, device="cuda")
            loop = batch(OLD_BITS, n, out)
            loop(); torch.cuda.synchronize()
            want = out.clone()
            if new_build:
                d.allow_fused = OLD_BITS | BATCH
                chunk, p1 = C.c_size_t(), C.c_int()
                assert L.ipk_pipeline_batches_previews(C.byref(d), 1, n, C.byref(chunk), C.byref(p1)) == 1 and p1.value == 1 and chunk.value == 64, name
                out.zero_()
                run = batch(OLD_BITS | BATCH, n, out)
                _lib.check(L.ipk_timing_begin(), "ipk_timing_begin")
                with ipa.launch_log() as ran:
                    run(); torch.cuda.synchronize()
                arr = (_lib.StageTime * 8)(); ns = C.c_int(0)
                _lib.check(L.ipk_timing_end(arr, 8, C.byref(ns)), "ipk_timing_end")
                assert ns.value == 2 and len([e for e in ran if "batch=1" in e]) == 1, (name, n, ns.value, sorted(ran))
                assert torch.equal(out, want), "%s, n = %d: the batch differs from this build's loop" % (name, n)
                if oracle and n == NS[0]:
                    for i in (0, n - 1):
                        assert np.array_equal(out[i * px3: (i + 1) * px3].cpu().numpy().reshape(fh, fw, 3), _oracle(util, frames[i], kind, w, h, mw)), \
                            "%s: frame %d differs from the oracle's" % (name, i)
                    res["oracle"] = 1
                res["batch"] = _wall(run, runs)
            res["loop"] = _wall(batch(OLD_BITS, n, out), runs)
            print("RESULT " + json.dumps(res), flush=True)
        del frames, pipe, rgbe
        torch.cuda.empty_cache()


def summarise(acc, rounds, runs):
    """acc: {(case, n): {"demosaic": ..., "oracle": ..., "t": {(build, key): [ms, ...]}}} -> the report's lines"""
    import numpy as np
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    lines = ["batch_previews_probe: noise frames, device-resident sources, 8-bit outputs into one allocation; %d rounds of (parent, new) as alternating child" % rounds,
             "processes on one box; wall clock around ipk_pipeline_run_batch and a synchronise, ms PER FRAME (the call's time / n), medians with the fastest run in",
             "brackets; %d runs per round, 3 warm-ups; spread = the parent's p95 - median, per frame.  parent = the parent build's ipk_pipeline_run_batch (its loop:" % runs,
             "two launches per frame; every bit it knows set); loop = this build with IPK_FUSED_BATCH_PREVIEWS clear; batch = this build with the bit set (two",
             "launches per 64 frames).  floor = the source's bytes per frame at %.1f TB/s." % HBM_TBS, ""]
    slower, outside, gains = [], [], {}
    for name, kind, w, h, mw in CASES:
        c0 = acc.get((name, 0))
        if c0 is None:
            continue
        floor = w * h * 2 / (HBM_TBS * 1e12) * 1e3
        lines.append("  %s (demosaic %s; %.0f MB per frame, floor %.4f ms)" % (name, c0.get("demosaic"), w * h * 2 / 1e6, floor))
        for n in NS:
            c = acc.get((name, n))
            if c is None or ("new", "batch") not in c["t"]:
                continue
            P, S, N = ([v / n for v in c["t"][(b, k)]] for b, k in (("parent", "loop"), ("new", "loop"), ("new", "batch")))
            if n >= 8 and med(N) > med(P) + spread(P):
                slower.append("%s at n = %d (batch %.4f ms per frame, parent %.4f, spread %.4f)" % (name, n, med(N), med(P), spread(P)))
            gains.setdefault(n, []).append(med(P) / med(N))
            lines.append("    n = %2d   parent %7.4f (%.4f; spread %.4f)  loop %7.4f (%.4f)  batch %7.4f (%.4f)   x%.2f over the parent%s"
                         % (n, med(P), low(P), spread(P), med(S), low(S), med(N), low(N), med(P) / med(N), "; checked against the oracle" if c.get("oracle") else ""))
        P, N = c0["t"][("parent", "single")], c0["t"][("new", "single")]
        inside = abs(med(N) - med(P)) <= spread(P)
        if not inside:
            outside.append("%s (%.4f -> %.4f ms, spread %.4f)" % (name, med(P), med(N), spread(P)))
        lines.append("    the single-frame general kernel, parent -> this build: %7.4f (%.4f; spread %.4f) -> %7.4f (%.4f)   %s"
                     % (med(P), low(P), spread(P), med(N), low(N), "inside the parent's spread" if inside else
                        ("FASTER than the parent beyond its spread" if med(N) < med(P) else "SLOWER than the parent beyond its spread")))
    lines += ["", "batch over the parent's loop, per frame, smallest .. largest over the cases: " +
              "; ".join("n = %d: x%.2f .. x%.2f" % (n, min(v), max(v)) for n, v in sorted(gains.items())),
              "single-frame launches outside the parent's spread: " + ("none" if not outside else "; ".join(outside)),
              "not measured: f32 sources, f32 and 16-bit outputs, scattered destinations, rasters and the window-8 geometries (pass 1 per frame), photo-like data",
              "cases at n >= 8 where the batch is SLOWER than the parent's loop beyond the parent's spread: " + ("none" if not slower else "; ".join(slower))]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_batch_previews.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new"]); ap.add_argument("--oracle", action="store_true")
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
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", label, "--runs", str(a.runs)]
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
