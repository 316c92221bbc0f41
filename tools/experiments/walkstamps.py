"""The walk / shade split of the 1-spp looping pass per bounce, and how many paths its waves hold (temporary -DPT_STAMPS build: apply
tools/experiments/walkstamps.patch to csrc/, `make EXTRA=-DPT_STAMPS`, keep the library as tools/experiments/libpt_stamps.so; the hooks are not
kept in the tree).  Every wave of the looping pass leaves one row: per trace -> shade iteration its s_memtime cycles in the walk and in the
shading step, its live paths, and whether the walk was the cooperative one.  C2, one frame at a time, the separate looping pass pinned.
usage: PT_HIP_LIB=tools/experiments/libpt_stamps.so [PT_COOP_WALK=0] python tools/experiments/walkstamps.py"""
import ctypes
import os
import sys

os.environ.setdefault("PT_FUSE_LOOP", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import dxrs_amd_loader  # noqa
import dxrs_amd
from dxrs_amd.types import graphics_settings

WAVES, ITERS = 4096, 8
lib = ctypes.CDLL(os.environ["PT_HIP_LIB"])
w, h = 1920, 1080
host = dxrs_amd.load_host()
spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
r = dxrs_amd.Renderer(device=0, frames_in_flight=1)
r.set_scene(spheres, materials, sd)
buf = torch.empty((h * w, 4), dtype=torch.float32, device="cuda")
rows = np.zeros((WAVES, ITERS, 4), dtype=np.uint32)


def frame(k):
    gs = graphics_settings(w, h, frame_index=k, bounces=8, spp=1)
    r.set_camera(host.camera(w, h, jitter_index=0))  # (a resting view: beam lists and region records, as in the throughput run)
    r.set_constants(gs)
    r.render_device(buf.data_ptr())


for k in range(6):
    frame(k)
acc = []
for k in range(6, 14):
    assert lib.pt_debug_stamps(None, 1) == 0
    frame(k)
    assert lib.pt_debug_stamps(ctypes.c_void_p(rows.ctypes.data), 0) == 0
    acc.append(rows.copy())
a = np.stack(acc).astype(np.float64)  # (frames, waves, iterations, 4)
ran = a[..., 2] > 0
print(f"PT_COOP_WALK={os.environ.get('PT_COOP_WALK', '(default)')}: {ran[:, :, 0].sum() / len(acc):.0f} waves per launch, {a[:, :, 0, 2].sum() / len(acc):.0f} paths")
print("iteration  waves  live/wave   walk cycles  shade cycles  walk share")
for it in range(ITERS):
    m = ran[:, :, it]
    if not m.any():
        break
    tr, sh = a[:, :, it, 0][m].mean(), a[:, :, it, 1][m].mean()
    print(f"{it:9d} {m.sum() / len(acc):6.0f} {a[:, :, it, 2][m].mean():10.1f} {tr:13.0f} {sh:13.0f} {tr / (tr + sh):10.2f}")
m = ran
print(f"all: walk {a[..., 0][m].sum() / (a[..., 0][m].sum() + a[..., 1][m].sum()):.2f} of the stamped cycles; per wave {a[..., 0].sum(axis=2)[ran[:, :, 0]].mean():.0f} walk + "
      f"{a[..., 1].sum(axis=2)[ran[:, :, 0]].mean():.0f} shade cycles; longest wave {(a[..., 0] + a[..., 1]).sum(axis=2).max():.0f}")
print("live paths   wave-iterations  share   walk cycles  cooperative")
for lo, hi in ((1, 1), (2, 8), (9, 16), (17, 32), (33, 64)):
    c = ran & (a[..., 2] >= lo) & (a[..., 2] <= hi)
    if c.any():
        print(f"{lo:3d}-{hi:<3d} {c.sum() / len(acc):18.0f} {c.sum() / ran.sum():7.2f} {a[..., 0][c].mean():12.0f} {a[..., 3][c].mean():10.2f}")
r.close()
