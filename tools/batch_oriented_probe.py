#!/usr/bin/env python
"""Development tool: what a shoot of thumbnails costs per frame when its files carry their own orientation as well as their own white balance and exposure.
The PARENT build offers such a caller one thing: a loop of ipk_pipeline_run over the per-frame descriptors (an oriented preview: the scaling pass, the
chain, the quantise and the transform).  This build's ipk_pipeline_run_batch_each with IPK_FUSED_BATCH_ORIENTED keeps the frames in one varied run: the
shared scaling launch and ONE point-wise launch per chunk whose records fold each frame's orientation into the walk.  An optional third build of the
same interface (--gather; tools/build_variant.sh) is timed beside the two: the second part of profiles/r21_batch_oriented.txt was taken while this build
still had a transposed tile walk (launch tag orient=2), with the same source and the walk compiled out as that third build -- the comparison that decided
against the walk, which has since been deleted.

Frames (noise, device-resident) under a SQUARE box, so that landscape and portrait frames negotiate one demosaic size: 24 MP RGGB u16 -> 256 and 400, 50 MP
X-Trans u16 -> 270, 24 MP mono u16 -> 256, each at n = 2, 8, 16, 64.  Batches: all Rotate90 ("rot90"); Normal and Rotate90 alternating ("mixed"); all
Normal ("normal": this build's own price of orientation).  Outputs: u8 everywhere, u16 for the Rotate90 batch as well.  Before
anything is timed the batch call is compared with this build's own loop of ipk_pipeline_run (all frames, equal bytes), the plan must say route 2 and the
launch log must show ONE carrier with the expected orient= tag.  Also the carriers' launches outside the mode, in every build: this build's all-Normal
varied batch, single-frame ipk_pointwise_chain_out at 2160x1440 and 6000x4000 to f32 and u8, and the cached-region gather launch over 1/16 of a 24 MP frame
(tools/batch_each_probe.py's).  Wall clock around the call and a stream synchronise, 3 warm-ups, medians and minima over all rounds; the builds alternate
as child processes of one session on one box; spread = a build's p95 - median.
usage: tools/batch_oriented_probe.py --parent /path/to/libparent.so [--gather /path/to/libnotile.so] [--out profiles/r21_batch_oriented.txt]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import batch_each_probe as bep                                             # the cases, the timing loop and the untouched launches are that tool's

CASES = [(name.replace("wide", "box"), kind, w, h, mw) for name, kind, w, h, mw in bep.CASES]
NS = bep.NS
OLD_BITS, BATCH, ORIENTED = 255, 256, 512
BATCHES = [("rot90", 1), ("mixed", 1), ("rot90", 2), ("normal", 1)]       # (the frames' orientations, out_type)
OUT_NAME = {1: "u8", 2: "u16"}


def worker(runs, label):
    """one build: a JSON line per case, batch kind and batch size"""
    import torch
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    import util
    ipa.init(0)
    L = ipa.lib()
    new = label != "parent"
    bep.untouched(runs, ipa, util, L, _lib)
    for ci, (name, kind, w, h, box) in enumerate(CASES):
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + 210 + ci)
        frames = [torch.randint(0, 16384, (w * h,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16) for _ in range(max(NS))]
        pipe = bep._pipe(ipa, util, kind, w, h, box, frames[0])
        pipe.globals.settings.maxheight = box
        (dw, dh), _ = pipe.sizes()
        st = torch.cuda.current_stream().cuda_stream
        for what, out_type in BATCHES:
            esz = out_type                                                  # u8: 1 byte, u16: 2
            px3 = dw * dh * 3 * esz
            descs = []
            for i in range(max(NS)):
                d = _lib.PipelineDesc.from_buffer_copy(pipe.desc())
                d.wb_coeffs[:], d.exposure = bep._settings(util, i)
                d.rotation = 1 if what == "rot90" or (what == "mixed" and i % 2) else 0
                descs.append(d)

            def set_mask(mask):
                for d in descs:
                    d.allow_fused = mask

            def loop(n, out):
                def run():
                    for i in range(n):
                        _lib.check(L.ipk_pipeline_run(C.byref(descs[i]), frames[i].data_ptr(), out.data_ptr() + i * px3, out_type, None, st), "ipk_pipeline_run")
                return run

            def each(n, out):
                dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
                sp = (C.c_void_p * n)(*[f.data_ptr() for f in frames[:n]])
                op = (C.c_void_p * n)(*[out.data_ptr() + i * px3 for i in range(n)])
                return lambda: _lib.check(L.ipk_pipeline_run_batch_each(dp, sp, op, n, out_type, None, st), "ipk_pipeline_run_batch_each")
            for n in NS:
                res = dict(case=name, what=what, out=out_type, n=n, demosaic="%dx%d" % (dw, dh))
                out = torch.zeros(n * px3, dtype=torch.uint8, device="cuda")
                set_mask(OLD_BITS)
                loop(n, out)(); torch.cuda.synchronize()
                want = out.clone()
                if new:
                    set_mask(OLD_BITS | BATCH | ORIENTED)
                    dp = (C.POINTER(_lib.PipelineDesc) * n)(*[C.pointer(d) for d in descs[:n]])
                    route = (C.c_int * n)()
                    _lib.check(L.ipk_pipeline_batch_each_plan(dp, n, out_type, route, None), "ipk_pipeline_batch_each_plan")
                    assert list(route) == [2] * n, (name, what, n, list(route))
                    out.zero_()
                    run = each(n, out)
                    with ipa.launch_log() as ran:
                        run(); torch.cuda.synchronize()
                    hits = [e for e in ran if "k_raster_chain<ipk::Rgbe32, %d>[" % out_type in e and "batch=1" in e]
                    assert len(hits) == 1 and (hits[0].endswith("batch=1]") if what == "normal" else ",orient=" in hits[0]), (name, what, n, sorted(ran))
                    assert torch.equal(out, want), "%s, %s, n = %d: the batch differs from this build's loop" % (name, what, n)
                    res["each"] = bep._wall(run, runs)
                else:
                    res["loop"] = bep._wall(loop(n, out), runs)
                print("RESULT " + json.dumps(res), flush=True)
        del frames, pipe
        torch.cuda.empty_cache()


def summarise(acc, builds, rounds, runs):
    import numpy as np
    med = lambda x: float(np.median(x))
    low = lambda x: float(np.min(x))
    spread = lambda x: float(np.percentile(x, 95)) - med(x)
    have_gather = "gather" in builds
    lines = ["batch_oriented_probe: noise frames, device-resident sources, results into one allocation, every frame with its own wb_coeffs and exposure, square size",
             "limits; %d rounds of (%s) as alternating child processes on one box; wall clock around the call(s) and a synchronise, ms PER FRAME (the time / n)," % (rounds, ", ".join(builds)),
             "medians with the fastest run in brackets; %d runs per round, 3 warm-ups; spread = that build's p95 - median, per frame.  parent = the parent build's only" % runs,
             "offer, a loop of ipk_pipeline_run over the per-frame descriptors (every bit it knows set); new = this build's ipk_pipeline_run_batch_each with",
             "IPK_FUSED_BATCH_ORIENTED (route 2: the shared scaling launch and ONE oriented point-wise launch per 64 frames); gather = the --gather",
             "build, where one was given.  rot90 = every frame Rotate90; mixed = Normal and Rotate90 alternating; normal = every",
             "frame Normal (this build's batch of r20: what orientation costs on top of it).", ""]
    verdict = []
    for name, kind, w, h, mw in CASES:
        for what, out_type in BATCHES:
            first = True
            for n in NS:
                c = acc.get((name, what, out_type, n))
                if c is None or ("new", "each") not in c["t"] or ("parent", "loop") not in c["t"]:
                    continue
                if first:
                    lines.append("  %s, %s -> %s (demosaic %s)" % (name, what, OUT_NAME[out_type], c.get("demosaic")))
                    first = False
                P, E = [v / n for v in c["t"][("parent", "loop")]], [v / n for v in c["t"][("new", "each")]]
                row = "    n = %2d   parent %7.4f (%.4f; spread %.4f)  new %7.4f (%.4f; spread %.4f)   x%.2f over the parent" % (
                    n, med(P), low(P), spread(P), med(E), low(E), spread(E), med(P) / med(E))
                flat = acc.get((name, "normal", out_type, n))
                if what != "normal" and flat is not None and ("new", "each") in flat["t"]:
                    row += ", %+.4f ms to the all-Normal batch" % (med(E) - med([v / n for v in flat["t"][("new", "each")]]))
                if have_gather and ("gather", "each") in c["t"]:
                    G = [v / n for v in c["t"][("gather", "each")]]
                    row += "; gather %7.4f (%.4f; spread %.4f)" % (med(G), low(G), spread(G))
                    if what == "rot90":
                        d, s = med(G) - med(E), max(spread(G), spread(E))
                        verdict.append((name, out_type, n, d, s))
                        row += ": new is %s" % ("FASTER beyond the spreads" if d > s else "SLOWER beyond the spreads" if -d > s else "inside the spreads")
                lines.append(row)
    lines += ["", "launches of the carrier kernels outside the mode, parent -> this build (ms, medians with the fastest run in brackets):"]
    for name in [c[0] for c in bep.CHAINS] + [bep.GATHER]:
        c = acc.get((name, "", 0, -1))
        if c is None or ("new", "single") not in c["t"] or ("parent", "single") not in c["t"]:
            lines.append("    %-44s not measured (the launch did not occur)" % name)
            continue
        P, N = c["t"][("parent", "single")], c["t"][("new", "single")]
        inside = abs(med(N) - med(P)) <= spread(P)
        lines.append("    %-44s %-40s %7.4f (%.4f; spread %.4f) -> %7.4f (%.4f)   %s"
                     % (name, c.get("kernel", "").replace("ipk::", ""), med(P), low(P), spread(P), med(N), low(N), "inside the parent's spread" if inside else
                        ("FASTER than the parent beyond its spread" if med(N) < med(P) else "SLOWER than the parent beyond its spread")))
    if verdict:
        lines += ["", "new against the --gather build, Rotate90 batches (gather - new, ms per frame; the larger of the two builds' spreads):"]
        lines += ["    %-34s -> %-3s n = %2d   %+.4f (spread %.4f)" % (nm, OUT_NAME[o], n, d, s) for nm, o, n, d, s in verdict]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--gather"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_batch_oriented.txt"))
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--worker", choices=["parent", "new", "gather"])
    ap.add_argument("--limit", type=int, default=400, help="seconds a worker may take")
    a = ap.parse_args()
    if a.worker:
        return worker(a.runs, a.worker)
    if not a.parent or not os.path.exists(a.parent):
        sys.exit("--parent: the parent commit's build of the library is the baseline")
    builds = [("parent", os.path.abspath(a.parent)), ("new", None)] + ([("gather", os.path.abspath(a.gather))] if a.gather else [])
    acc = {}
    for rnd in range(a.rounds):
        for label, so in builds:
            env = dict(os.environ)
            env.pop("IPK_SO_OVERRIDE", None)
            if so:
                env["IPK_SO_OVERRIDE"] = so
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", label, "--runs", str(a.runs)]
            p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            seen = []
            for line in p.stdout:                                           # read as they come, so that a long case still shows progress
                seen.append(line)
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    print("  round %d %s: %s %s n = %d" % (rnd, label, r["case"], r.get("what", ""), r["n"]), flush=True)
            if p.wait() != 0:
                sys.stderr.write("".join(seen))
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (label, p.returncode))
            for line in seen:
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault((r["case"], r.get("what", ""), r.get("out", 0), r["n"]), dict(t={}))
                    for k, v in r.items():
                        if isinstance(v, list):
                            c["t"].setdefault((label, k), []).extend(v)
                        elif k not in ("case", "n", "what", "out"):
                            c[k] = v
    lines = summarise(acc, [b[0] for b in builds], a.rounds, a.runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
