#!/usr/bin/env python
"""Development tool: what an active OpRotateCrop costs on the staged route and on the one-launch route (ipk_pipeline_desc.fuse_rotatecrop).
Times ipk_pipeline_run with device events on the launch stream in the steady state, a synchronise behind every timed run; the baseline is ANOTHER
BUILD of the library (the parent commit's: tools/build_variant.sh makes one), so the two builds alternate as child processes of one session on one
box: parent, this, parent, this, ...  Per case: medians over all rounds, the parent's own spread (p95 - median) and the acceptance "the new route's
median is below the parent's by more than that spread"; then the stage times ipk_timing reports for both routes.
usage: tools/rotatecrop_probe.py --parent /path/to/libparent.so [--out profiles/r08_rotatecrop.txt] [--runs 100] [--rounds 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

CROP5 = (0.05, 0.05, 0.05, 0.05, 0.0)
ROT30 = (0.0, 0.0, 0.0, 0.0, 1.0 / 30.0)
# (label, width, height, f32 source?, out_type, rotatecrop)
CASES = [("%s %s %s" % (mp, io, rn), w, h, isf, ot, rc)
         for mp, w, h in (("24MP", 6000, 4000), ("100MP", 10000, 10000))
         for io, isf, ot in (("f32->f32", True, 0), ("u16->u8", False, 1))
         for rn, rc in (("crop 5%", CROP5), ("rot 1/30", ROT30))]


def worker(runs, new_build):
    """one build (the library IPK_SO_OVERRIDE names, or the tree's): a JSON line per case"""
    import numpy as np
    import torch
    import imagepipe_amd as ipa
    import util
    from imagepipe_amd import _lib
    ipa.init(0)
    L = ipa.lib()
    st = torch.cuda.current_stream().cuda_stream
    for label, w, h, isf, ot, rc in CASES:
        g = torch.Generator(device="cuda"); g.manual_seed(util.SEED + w)
        v = torch.randint(0, 16384, (h * w,), device="cuda", generator=g, dtype=torch.int32)      # noise data
        data = v.to(torch.float32) if isf else v.to(torch.int16)
        del v
        pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=data, cfa="RGGB", is_float=isf, blacklevels=[util.BLACK] * 4,
                                                         whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
        r = pipe.ops.rotatecrop
        r.crop_top, r.crop_right, r.crop_bottom, r.crop_left, r.rotation = [float(np.float32(x)) for x in rc]
        _, (fw, fh) = pipe.sizes()
        out = torch.empty(fw * fh * 3, dtype={0: torch.float32, 1: torch.uint8}[ot], device="cuda")
        res = dict(case=label, out="%dx%d" % (fw, fh))
        outs = {}
        for flag in ((0, 1) if new_build else (0,)):
            pipe.fuse_rotatecrop = bool(flag)
            d = pipe.desc()
            used = C.c_int(0)
            run = lambda: L.ipk_pipeline_run(C.byref(d), data.data_ptr(), out.data_ptr(), ot, C.byref(used), st)
            for _ in range(5):
                _lib.check(run(), "ipk_pipeline_run")
            torch.cuda.synchronize()
            assert used.value == flag, "%s: flag %d ran with used_fused = %d" % (label, flag, used.value)
            outs[flag] = out.clone()
            ts = []
            for _ in range(runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); run(); e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            res["flag%d" % flag] = ts
            stages = {}
            for _ in range(9):
                _, sl = pipe.run_timed(ot)
                for name, ms in sl:
                    stages.setdefault(name, []).append(ms)
            res["stages%d" % flag] = {k: float(np.median(x)) for k, x in stages.items()}
        if new_build:
            assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), label + ": the two routes disagree"
        print("RESULT " + json.dumps(res), flush=True)
        del pipe, data, out, outs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_rotatecrop.txt"))
    ap.add_argument("--runs", type=int, default=100); ap.add_argument("--rounds", type=int, default=2)
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
                    c = acc.setdefault(r["case"], dict(out=r["out"], parent=[], flag0=[], flag1=[], st_parent={}, st0={}, st1={}))
                    if which == "parent":
                        c["parent"] += r["flag0"]; c["st_parent"] = r["stages0"]
                    else:
                        c["flag0"] += r["flag0"]; c["flag1"] += r["flag1"]; c["st0"] = r["stages0"]; c["st1"] = r["stages1"]
            print("round %d %s done" % (rnd, which), flush=True)
    lines = ["rotatecrop_probe: ipk_pipeline_run, device events on the launch stream, a synchronise behind every timed run, 5 warm-ups; RGGB noise frames;",
             "%d rounds of (parent build, this build) as alternating child processes, %d runs per case and round: medians over %d runs" % (a.rounds, a.runs, a.rounds * a.runs),
             "spread = the parent's p95 - median; accepted = parent median - flag 1 median > spread", ""]
    ok_all = True
    for label, *_ in CASES:
        c = acc[label]
        mp, m0, m1 = (float(np.median(c[k])) for k in ("parent", "flag0", "flag1"))
        spread = float(np.percentile(c["parent"], 95)) - mp
        ok = mp - m1 > spread
        ok_all = ok_all and ok
        lines.append("%-26s -> %-11s parent %.4f ms (spread %.4f)  flag 0 %.4f ms  flag 1 %.4f ms  speed-up %.2fx  %s"
                     % (label, c["out"], mp, spread, m0, m1, mp / m1, "accepted" if ok else "NOT accepted"))
        lines.append("    parent stages: " + ", ".join("%s %.4f" % kv for kv in c["st_parent"].items()))
        lines.append("    flag 1 stages: " + ", ".join("%s %.4f" % kv for kv in c["st1"].items()))
    lines.append("")
    lines.append("every case accepted" if ok_all else "NOT every case accepted")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
