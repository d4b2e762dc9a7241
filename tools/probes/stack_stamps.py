"""Phase timing inside stack_fused_kernel<.., true> (measurement build: -DSF_STAMPS=<worker> on the source with
tools/probes/stack_fused_probes.patch applied).
    make -C locator_amd/csrc stack_probe TAG=sfstamps XDEF=-DSF_STAMPS=0
    python3 tools/probes/stack_stamps.py build/liblocator_hip_sfstamps.so [width]
Prints, per layer pass of one worker of the last training launch (shader cycles, median over its waves, min..max where it
matters): pass entered -> slot 0 consumed (the epilogue operands' issue, the wait for the slot's rows and its FMAs), each
further slot of the last trip round the ring (wait + FMAs + the previous slot's request), the barrier behind the contraction +
the operand wait, the epilogue + second barrier, and the whole pass.  A wave has no request outstanding only between the
moment its last in-flight slot lands and its next request; with every slot re-requested when consumed that cannot happen
while a pass runs, so the stamps show where a wave WAITS instead: the slot columns."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from locator_amd import _lib

path = os.path.abspath(sys.argv[1])
_lib.use_library(path)
import torch

from locator_amd.net import LocatorNet, upload_genotypes
from locator_amd.synth import normalize_locs, split_indices, synth_genotypes
from locator_amd.train import FitLoop

width = int(sys.argv[2]) if len(sys.argv) > 2 else 256
K, n = 100_000, 1000
x, locs = synth_genotypes(n, K, seed=20260101, n_na=n // 10)
ynorm = normalize_locs(locs)[4]
train, test, pred = split_indices(locs, seed=12345)
X = upload_genotypes(x, "cuda:0")
Y = torch.from_numpy(np.nan_to_num(np.asarray(ynorm)).astype(np.float32)).to("cuda:0")
net = LocatorNet(X, Y, K, width, 10, 0.25, seed=12345, device="cuda:0")
rng = np.random.default_rng(99)
loop = FitLoop(net, train, test, batch_size=32, max_epochs=200, patience=10 ** 6, lr_patience=16, use_graph=True,
               perm_fn=lambda e: rng.permutation(len(train)), depth=2, xchain=True)
for _ in range(8):
    loop.submit(None)
    loop.collect(None)
loop.collect(0)
torch.cuda.synchronize()
PASSES = 40
buf = (C.c_ulonglong * (8 * PASSES * 12))()
lib = C.CDLL(path)
assert lib.loc_debug_stack_stamps(buf) == 0
s = np.array(buf[:], dtype=np.uint64).reshape(8, PASSES, 12).astype(np.int64)
n_pass = int((s[0, :, 11] > 0).sum())
ns = int((s[0, 0, 1:9] > 0).sum())                      # slots of the ring at this width
print(f"width {width}: {n_pass} passes stamped, {ns} slots; entry of each wave relative to the earliest:",
      (s[:, 0, 0] - s[:, 0, 0].min()).tolist())
print("pass  total | enter->slot0 | " + " | ".join(f"slot{j}" for j in range(1, ns)) + " | barrier+operands | epilogue")
med = lambda a: int(np.median(a))
tot = []
for p in range(n_pass):
    t = s[:, p]
    whole = (s[:, p + 1, 0] - t[:, 0]) if p + 1 < n_pass else (t[:, 10] - t[:, 0])
    first = t[:, 1] - t[:, 0]
    slots = [t[:, 1 + j] - t[:, j] for j in range(1, ns)]
    bar = t[:, 9] - t[:, ns]
    epi = t[:, 10] - t[:, 9]
    tot.append([med(whole), med(first)] + [med(v) for v in slots] + [med(bar), med(epi)])
    print(f"{p:3d} {med(whole):7d} | {int(first.min())}..{int(first.max())} | " + " | ".join(str(med(v)) for v in slots) +
          f" | {int(bar.min())}..{int(bar.max())} | {med(epi)}")
tot = np.array(tot)
print("median over the passes:", np.median(tot, axis=0).astype(int).tolist())
print("first pass entered -> last epilogue done, per wave:", (s[:, n_pass - 1, 10] - s[:, 0, 0]).tolist())
