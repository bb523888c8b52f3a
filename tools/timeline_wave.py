"""Debug: per-unit timeline of the wave-autonomous matrix-core render kernel (-DGF_TIMELINE=1 build).
python tools/timeline_wave.py [config]"""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, ".")
from gaussianformer_amd import build as _b
_tl = os.environ.get("GF_TIMELINE_LIB") or os.path.join(_b.CSRC, "libgf_hip_timeline.so")   # (another -DGF_TIMELINE=1 build: an A/B)
_deps = [os.path.join(_b.CSRC, f) for f in _b.SOURCES + _b.HEADERS]
if "GF_TIMELINE_LIB" not in os.environ and (not os.path.exists(_tl) or any(os.path.getmtime(d) > os.path.getmtime(_tl) for d in _deps if os.path.exists(d))):
    _b.build(extra_flags=("-DGF_TIMELINE=1",), lib_name="libgf_hip_timeline.so")
os.environ["GF_LIB"] = _tl
from gaussianformer_amd import _lib
from gaussianformer_amd.local_aggregate import SplatForwardPlan
from gaussianformer_amd.synthetic import make_splat_inputs
import oracle
config = sys.argv[1] if len(sys.argv) > 1 else "nuscenes_gs25600_solid"
dev = torch.device("cuda:0")
si = make_splat_inputs(config, seed=0)
pi, mi, radii, cov6 = oracle.prepare_splat_inputs(si.pts, si.means3D, si.scales, si.cov3D, si.pc_min, si.grid_size, si.scale_multiplier)
t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (si.pts, pi, si.means3D, mi, si.opacities, si.semantics, radii, cov6)]
plan = SplatForwardPlan(0, *t, si.H, si.W, si.D, flags=1)
lib = _lib.load()
for _ in range(5): plan.run()
torch.cuda.synchronize()
nu = 8 * ((si.H + 7) // 8) * ((si.W + 7) // 8) * 4 * ((si.D + 7) // 8) // 8 + 64
tl = torch.zeros(8 * nu, dtype=torch.int64, device=dev)
lib.gf_debug_set_timeline.argtypes = [ctypes.c_void_p]
lib.gf_debug_set_timeline(tl.data_ptr())
# ... and of the records pass: a start and an end stamp per wave (P / 64 record waves + the point scans' waves), same clock
ptl = torch.zeros(2 * (plan.P // 64 + 8192), dtype=torch.int64, device=dev)
lib.gf_debug_set_prep_timeline.argtypes = [ctypes.c_void_p]
lib.gf_debug_set_prep_timeline(ptl.data_ptr())
plan.run(); torch.cuda.synchronize()
lib.gf_debug_set_timeline(None)
lib.gf_debug_set_prep_timeline(None)
PT = ptl.cpu().numpy().reshape(-1, 2).astype(np.float64)
PT = PT[PT[:, 0] > 0]
T = tl.cpu().numpy().reshape(nu, 8).astype(np.float64)
os.makedirs("gpurun_out", exist_ok=True)
np.save("gpurun_out/timeline_wave_%s.npy" % config, T)
idx = np.nonzero(T[:, 0] > 0)[0]   # unit index inside an XCD (the eight XCDs write the same rows: the last one stays)
T = T[idx]
took = T[:, 7] >= 1000             # short rows: the unit took its supertile's list from unit 0 (the groups are counted below 1000)
groups = T[:, 7] % 1000
first = idx // (((si.H + 7) // 8) * ((si.W + 7) // 8) + 7 >> 3) == 0   # ... dealt r-major: the first ceil(nsuper / 8) are the units 0
t0 = T[:, 0].min()
T = (T[:, :7] - t0) / 100.0
print("units", len(T), "kernel span us %.2f" % T[:, 6].max(), " groups per unit %.2f" % groups.mean())
if len(PT):
    # the step's pieces inside one call: records pass span, the boundary behind it, render span (min start to max end, 100 MHz clock)
    print("records pass: waves %d, span us %.2f (wave mean %.2f, p90 %.2f); last end -> first render start us %.2f" % (
        len(PT), (PT[:, 1].max() - PT[:, 0].min()) / 100.0, ((PT[:, 1] - PT[:, 0]) / 100.0).mean(),
        np.percentile((PT[:, 1] - PT[:, 0]) / 100.0, 90), (t0 - PT[:, 1].max()) / 100.0))
names = ["row landed", "list built", "boxes landed", "first records landed", "consumed", "stored"]
prev = T[:, 0]
for k, nme in enumerate(names, 1):
    cur = np.where(T[:, k] > 0, T[:, k], prev)
    d = cur - prev
    print(f"{nme:22s} +{d.mean():6.2f} us (p50 {np.median(d):5.2f}, p90 {np.percentile(d, 90):5.2f}, max {d.max():5.2f})")
    prev = cur
lb = np.where(T[:, 2] > 0, T[:, 2], T[:, 1]) - T[:, 1]
bx = np.where(T[:, 3] > 0, T[:, 3], T[:, 2]) - T[:, 1]
for nme, m in (("units 0 (publish)", first), ("took unit 0's list", took), ("built their own list", ~took & ~first)):
    if m.any():
        print(f"{nme:22s} {m.sum():5d} units ({100.0 * m.mean():4.1f} %): list built +{lb[m].mean():5.2f} us, row landed -> boxes landed {bx[m].mean():5.2f} us, "
              f"unit total {(T[m, 6] - T[m, 0]).mean():5.2f} us, started p50 {np.median(T[m, 0]):5.2f} us")
tot = T[:, 6] - T[:, 0]
print("unit total mean %.2f p50 %.2f p90 %.2f max %.2f" % (tot.mean(), np.median(tot), np.percentile(tot, 90), tot.max()))
st = np.sort(T[:, 0]); en = np.sort(T[:, 6])
print("starts: first 2048 by %.2f us; last unit starts %.2f; ends p50 %.2f p90 %.2f p99 %.2f max %.2f" % (st[min(2047, len(st) - 1)], st[-1], np.median(en), np.percentile(en, 90), np.percentile(en, 99), en.max()))
busy = tot.sum() / 2048.0
print("sum of unit times / 2048 slots = %.2f us" % busy)
