#!/usr/bin/env python
"""Development tool: what a frame whose filter has a fourth colour (RGBE) costs on the staged route and on the one-launch route
(ipk_pipeline_desc.allow_fused bit 1, IPK_FUSED_FOUR_COLOUR) -- and, because that route lives inside the generic-CFA variants of k_fused_bayer as a
run-time mode, whether X-Trans frames on their ordinary one-launch route kept their speed.
Times ipk_pipeline_run with device events on the launch stream in the steady state, a synchronise behind every timed run; the baseline is ANOTHER
BUILD of the library (the parent commit's: tools/build_variant.sh makes one from the parent's sources), so the two builds alternate as child
processes of one session on one box: parent, this, parent, this, ...  Each RGBE case is checked bit-identical to the staged route before it is
timed.  Per case: medians over all rounds, the parent's own spread (p95 - median) and the acceptance -- RGBE: "the one-launch median is below the
parent's staged median by more than that spread"; X-Trans: "this build's median is not above the parent's by more than that spread" --, then the
stage times ipk_timing reports.
usage: tools/fourcolour_probe.py --parent /path/to/libparent.so [--out profiles/r11_fourcolour.txt] [--runs 60] [--rounds 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
IO = [("f32->f32", True, 0), ("u16->u8", False, 1)]
RGBE_CASES = [("%s RGBE %s" % (name, io), w, h, "RGBE", isf, ot) for name, w, h in (("24MP 6000x4000", 6000, 4000), ("100MP 10000x10000", 10000, 10000))
              for io, isf, ot in IO]
XT_CASES = [("%s X-Trans %s" % (name, io), w, h, XT, isf, ot) for name, w, h in (("26MP 6240x4160", 6240, 4160), ("50MP 8736x5856", 8736, 5856))
            for io, isf, ot in IO]
# the same without a base curve: off the common parameter set, so on the runtime-flag variants (CM = 0) -- the instantiations whose code holds the new mode
XT_RT_CASES = [("%s X-Trans, no curve %s" % (name, io), w, h, XT, isf, ot) for name, w, h in (("26MP 6240x4160", 6240, 4160), ("50MP 8736x5856", 8736, 5856))
               for io, isf, ot in IO]


def _time(run, runs):
    import torch
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def _measure(ipa, pipe, data, ot, flags, runs, label, want_fused):
    """per flag value (Pipeline.fuse_four_colour): warm up, keep the output, time, then the stage times; the flag-1 output must equal the flag-0
    output BEFORE anything is timed"""
    import numpy as np
    import torch
    from imagepipe_amd import _lib
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    _, (fw, fh) = pipe.sizes()
    out = torch.empty(fw * fh * 3, dtype={0: torch.float32, 1: torch.uint8}[ot], device="cuda")
    res = dict(case=label, out="%dx%d" % (fw, fh))
    runners, outs = {}, {}
    for flag in flags:
        pipe.fuse_four_colour = bool(flag)
        d = pipe.desc()
        used = C.c_int(0)
        run = (lambda d=d, used=used: L.ipk_pipeline_run(C.byref(d), data.data_ptr(), out.data_ptr(), ot, C.byref(used), st))
        for _ in range(5):
            _lib.check(run(), "ipk_pipeline_run")
        torch.cuda.synchronize()
        assert used.value == want_fused(flag), "%s: flag %d ran with used_fused = %d" % (label, flag, used.value)
        outs[flag] = out.clone()
        runners[flag] = run
    if len(flags) == 2:
        assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), label + ": the two routes disagree"
    outs.clear()
    for flag in flags:
        pipe.fuse_four_colour = bool(flag)
        res["flag%d" % flag] = _time(runners[flag], runs)
        stages = {}
        for _ in range(7):
            _, sl = pipe.run_timed(ot)
            for name, ms in sl:
                stages.setdefault(name, []).append(ms)
        res["stages%d" % flag] = {k: float(np.median(x)) for k, x in stages.items()}
    print("RESULT " + json.dumps(res), flush=True)


def worker(runs, new_build):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case"""
    import torch
    import imagepipe_amd as ipa
    import util
    ipa.init(0)
    cm = util.cam_matrix().copy()
    cm[:, 3] = [0.05, -0.03, 0.08]                                       # the E channel counts

    def source(w, h, isf, cfa):
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + w)
        v = torch.randint(0, 16384, (h * w,), device="cuda", generator=g, dtype=torch.int32)      # noise data
        data = v.to(torch.float32) if isf else v.to(torch.int16)
        pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=data, cfa=cfa, is_float=isf, blacklevels=[util.BLACK] * 4,
                                                         whitelevels=[util.WHITE] * 4, wb_coeffs=(2.0, 1.0, 1.5, 1.3), cam_to_xyz_normalized=cm))
        return data, pipe

    for label, w, h, cfa, isf, ot in RGBE_CASES:
        data, pipe = source(w, h, isf, cfa)
        # the parent has no such route (and reads bit 1 of allow_fused as "on"): its staged run is the baseline
        _measure(ipa, pipe, data, ot, (0, 1) if new_build else (0,), runs, label, lambda flag: flag)
        del pipe, data
        torch.cuda.empty_cache()
    for label, w, h, cfa, isf, ot in XT_CASES + XT_RT_CASES:
        data, pipe = source(w, h, isf, cfa)
        if "no curve" in label:
            pipe.ops.basecurve.points = []
        _measure(ipa, pipe, data, ot, (0,), runs, label, lambda flag: 1)                              # both builds: the ordinary one-launch route
        del pipe, data
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_fourcolour.txt"))
    ap.add_argument("--runs", type=int, default=60); ap.add_argument("--rounds", type=int, default=2)
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", which, "--runs", str(a.runs)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("the %s worker failed (exit %d): nothing further is started" % (which, p.returncode))
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    c = acc.setdefault(r["case"], dict(out=r["out"], t={}, st={}))
                    for flag in (0, 1):
                        if "flag%d" % flag in r:
                            c["t"].setdefault((which, flag), []).extend(r["flag%d" % flag])
                            c["st"][(which, flag)] = r["stages%d" % flag]
            print("round %d %s done" % (rnd, which), flush=True)
    med = lambda x: float(np.median(x))
    stages = lambda d: ", ".join("%s %.4f" % kv for kv in d.items())
    lines = ["fourcolour_probe: ipk_pipeline_run, device events on the launch stream, a synchronise behind every timed run, 5 warm-ups; noise frames;",
             "%d rounds of (parent build, this build) as alternating child processes, %d runs per case and round: medians over %d runs" % (a.rounds, a.runs, a.rounds * a.runs),
             "spread = the parent's p95 - median", "",
             "IPK_FUSED_FOUR_COLOUR (new route; each case bit-identical to the staged route before it was timed): accepted = parent staged median - flag 1 median > spread"]
    ok_all = True
    for label, *_ in RGBE_CASES:
        c = acc[label]
        mp, m0, m1 = med(c["t"][("parent", 0)]), med(c["t"][("new", 0)]), med(c["t"][("new", 1)])
        spread = float(np.percentile(c["t"][("parent", 0)], 95)) - mp
        ok = mp - m1 > spread
        ok_all = ok_all and ok
        lines.append("%-36s -> %-11s parent %.4f ms (spread %.4f)  flag 0 %.4f ms  flag 1 %.4f ms  speed-up %.2fx  %s"
                     % (label, c["out"], mp, spread, m0, m1, mp / m1, "accepted" if ok else "NOT accepted"))
        lines.append("    parent stages: " + stages(c["st"][("parent", 0)]))
        lines.append("    flag 1 stages: " + stages(c["st"][("new", 1)]))
    lines += ["", "X-Trans on the ordinary one-launch route, both builds: accepted = this build's median - parent median <= spread",
              "(default curve: the common-parameter variants, whose code did not change; no curve: the runtime-flag variants, which carry the new mode)"]
    for label, *_ in XT_CASES + XT_RT_CASES:
        c = acc[label]
        mp, m1 = med(c["t"][("parent", 0)]), med(c["t"][("new", 0)])
        spread = float(np.percentile(c["t"][("parent", 0)], 95)) - mp
        ok = m1 - mp <= spread
        ok_all = ok_all and ok
        lines.append("%-36s -> %-11s parent %.4f ms (spread %.4f)  this build %.4f ms  ratio %.3f  %s"
                     % (label, c["out"], mp, spread, m1, m1 / mp, "accepted" if ok else "NOT accepted"))
        lines.append("    parent stages: " + stages(c["st"][("parent", 0)]))
        lines.append("    this build's : " + stages(c["st"][("new", 0)]))
    lines.append("")
    lines.append("every case accepted" if ok_all else "NOT every case accepted")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
