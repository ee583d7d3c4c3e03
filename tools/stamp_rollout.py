"""Diagnostic: where k_rollout's waves spend their cycles (s_memtime deltas per phase mark), from a -DDDZ_STAMP build of the
engine.  Not product.
  python tools/stamp_rollout.py [--lib STAMP_BUILD.so] [TABLES[,TABLES...]] [ITERS]
Without --lib the stamp build is compiled into build_variants/stamp.so first.  One launch of ITERS lock-step iterations
(default 200) is stamped per table count (default 65536,4096) after a 300-iteration warm-up; every wave adds up the cycles
between two marks of its own instruction stream, so a share below is a share of WAVE cycles (issue + waiting), not of time."""
import ctypes as C
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
lib = None
if len(args) >= 2 and args[0] == "--lib":
    lib = os.path.abspath(args[1])
    args = args[2:]
if lib is None:
    out = os.path.join(ROOT, "build_variants")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "stamp.so")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-DDDZ_STAMP=1", "-o", lib,
                           os.path.join(ROOT, "doudizhu-rl_amd", "csrc", "ddz_engine.hip")])
importlib.import_module("doudizhu-rl_amd._lib").use_library(lib)
import numpy as np  # noqa: E402
import torch  # noqa: E402

pkg = importlib.import_module("doudizhu-rl_amd")
raw = C.CDLL(lib)
raw.ddz_debug_set_stamps.argtypes = [C.c_void_p]
# the marks of k_rollout (csrc/ddz_engine.hip); a mark's cycles are those since the previous mark of the wave
NAMES = {
    0: "prologue / previous table's tail",
    1: "per-iteration setup (draws, hand / info select)",
    5: "follow of single / pair / triple: list + pick",
    11: "other closed-form list (lead, rare follow): list + pick",
    2: "hybrid: closed-form round + planner + scan rounds",
    3: "hybrid: flush of the staged rows",
    10: "hybrid: pick",
    6: "row updates",
    7: "carried scalars",
    8: "deal / turn change",
    4: "record store + end of iteration",
    9: "state store",
}
tables = [int(x) for x in (args[0].split(",") if args else ["65536", "4096"])]
iters = int(args[1]) if len(args) > 1 else 200
for T in tables:
    env = pkg.BatchedEnv(T, seed=0, want_ids=False)
    env.reset()
    env.rollout_random(300)
    torch.cuda.synchronize()
    buf = torch.zeros((T, 16), dtype=torch.int64, device="cuda")
    assert raw.ddz_debug_set_stamps(C.c_void_p(buf.data_ptr())) == 0
    env.rollout_random(iters)
    torch.cuda.synchronize()
    assert raw.ddz_debug_set_stamps(None) == 0
    s = buf.cpu().numpy().astype(np.float64)[:, :12]
    s = s[s.sum(1) > 0]   # one slot per wave: that of its first table
    tot = s.sum()
    print(f"T={T}: {len(s)} waves, {T / len(s):.1f} tables per wave, {iters} iterations; "
          f"{tot / (T * iters):.0f} wave cycles per table-iteration; status {env.status()}")
    for k in (0, 1, 5, 11, 2, 3, 10, 6, 7, 8, 4, 9):
        print(f"  mark {k:2d}  {100 * s[:, k].sum() / tot:6.2f} %  {s[:, k].sum() / (T * iters):7.1f} cycles per table-iteration  {NAMES[k]}")
    del env
