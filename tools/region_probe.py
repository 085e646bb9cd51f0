#!/usr/bin/env python
"""Development tool: what a region of the result costs against the whole frame (ipk_pipeline_run_region vs ipk_pipeline_run).  Every case is
first checked bit for bit against the slice of a whole run; then whole and region runs alternate in this one process, each timed with device
events (host forms: wall clock around the synchronous call), median of N after a warm-up.
usage: tools/region_probe.py [out.txt] [N]          (default profiles/r07_region.txt, N = 50)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import imagepipe_amd as ipa
import util
from imagepipe_amd import _lib

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_region.txt")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ipa.init(0)
L = ipa.lib()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def frame(W, H, cfa, is_float, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    v = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32)
    data = v.to(torch.float32) if is_float else v.to(torch.int16)
    return ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa=cfa, is_float=is_float, blacklevels=[util.BLACK] * 4,
                                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))


def device_case(label, W, H, cfa, is_float, out_type):
    pipe = frame(W, H, cfa, is_float, util.SEED + W)
    d = pipe.desc()
    src = pipe.globals.image.data.data_ptr()
    dt = {0: torch.float32, 1: torch.uint8, 2: torch.int16}[out_type]
    full = torch.empty(W * H * 3, dtype=dt, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    used, win = C.c_int(0), C.c_int(0)
    whole = lambda: L.ipk_pipeline_run(C.byref(d), src, full.data_ptr(), out_type, C.byref(used), st)
    _lib.check(whole(), "ipk_pipeline_run"); torch.cuda.synchronize()
    fv = full.view(H, W, 3)
    regions = [("whole frame as region", 0, 0, W, H), ("2560x1440 centre", (W - 2560) // 2, (H - 1440) // 2, 2560, 1440),
               ("2560x1440 corner", W - 2560, H - 1440, 2560, 1440), ("512x512 tile", 1024, 1536, 512, 512), ("one full-width row", 0, H // 2, W, 1)]
    say("%s: %dx%d %s %s -> %s" % (label, W, H, "X-Trans" if cfa == XT else cfa, "f32" if is_float else "u16", {0: "f32", 1: "u8", 2: "u16"}[out_type]))
    for name, x, y, w, h in regions:
        reg = torch.empty(w * h * 3, dtype=dt, device="cuda")
        run = lambda: L.ipk_pipeline_run_region(C.byref(d), src, x, y, w, h, reg.data_ptr(), out_type, C.byref(win), st)
        _lib.check(run(), "ipk_pipeline_run_region"); torch.cuda.synchronize()
        same = torch.equal(fv[y:y + h, x:x + w].contiguous().view(-1).view(torch.uint8), reg.view(torch.uint8))
        assert same, "%s %s: region differs from the slice of the whole run" % (label, name)
        for _ in range(5):
            whole(); run()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(N)]
        for e in ev:                                        # alternating: whole, region, whole, region, ...
            e[0].record(); whole(); e[1].record(); e[2].record(); run(); e[3].record()
        torch.cuda.synchronize()
        tw = float(np.median([e[0].elapsed_time(e[1]) for e in ev])); tr = float(np.median([e[2].elapsed_time(e[3]) for e in ev]))
        say("  %-22s windowed=%d  whole %.4f ms  region %.4f ms  region/whole %.3f  (area %.4f)" % (name, win.value, tw, tr, tr / tw, w * h / (W * H)))
    del full


def host_case(W, H):
    pipe = frame(W, H, "RGGB", False, util.SEED + 7)
    d = pipe.desc()
    hs = L.ipk_host_alloc(W * H * 2); hd = L.ipk_host_alloc(W * H * 3); hr = L.ipk_host_alloc(2560 * 1440 * 3)
    try:
        frame_host = pipe.globals.image.data.cpu().numpy()          # kept alive across the copy
        C.memmove(hs, frame_host.ctypes.data, W * H * 2)
        x, y, w, h = (W - 2560) // 2, (H - 1440) // 2, 2560, 1440
        used, win = C.c_int(0), C.c_int(0)
        whole = lambda: _lib.check(L.ipk_host_pipeline_run(C.byref(d), hs, hd, 1, C.byref(used)), "ipk_host_pipeline_run")
        run = lambda: _lib.check(L.ipk_host_pipeline_run_region(C.byref(d), hs, x, y, w, h, hr, 1, C.byref(win)), "ipk_host_pipeline_run_region")
        whole(); run()
        a = np.ctypeslib.as_array((C.c_uint8 * (W * H * 3)).from_address(hd)).reshape(H, W, 3)
        b = np.ctypeslib.as_array((C.c_uint8 * (w * h * 3)).from_address(hr)).reshape(h, w, 3)
        assert np.array_equal(a[y:y + h, x:x + w], b), "host region differs from the slice of the whole run"
        for _ in range(5):
            whole(); run()
        tw, tr = [], []
        for _ in range(N):
            t0 = time.perf_counter(); whole(); t1 = time.perf_counter(); run(); t2 = time.perf_counter()
            tw.append(t1 - t0); tr.append(t2 - t1)
        mw, mr = 1e3 * float(np.median(tw)), 1e3 * float(np.median(tr))
        say("host -> host: %dx%d RGGB u16 -> u8, page-locked (ipk_host_alloc) buffers" % (W, H))
        say("  ipk_host_pipeline_run (whole) %.3f ms   ipk_host_pipeline_run_region 2560x1440 centre windowed=%d %.3f ms   speed-up %.2fx"
            % (mw, win.value, mr, mw / mr))
    finally:
        L.ipk_host_free(hs); L.ipk_host_free(hd); L.ipk_host_free(hr)


say("region_probe: device-event medians of %d alternating whole / region runs after 5 warm-ups; every region checked against the whole run first" % N)
say("device: %s" % torch.cuda.get_device_name(0))
device_case("100 MP headline", 10000, 10000, "RGGB", True, 0)
device_case("100 MP", 10000, 10000, "RGGB", False, 1)
device_case("50 MP X-Trans", 8664, 5776, XT, False, 1)
host_case(6000, 4000)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, "w").write("\n".join(lines) + "\n")
print("wrote", OUT)
