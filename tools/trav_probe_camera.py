"""Developer probe: tools/trav_probe.py's report for a camera-rays-only render of C4 (the normals visualiser, one un-jittered ray per pixel):
what k_extend executes per camera ray, with the entry nodes of device/entry_nodes.h or without.  Needs a library built with
-DPBRS_PROBE_TRAV (tools/ablate.sh) selected through PBRS_GPU_LIB.     python tools/trav_probe_camera.py 1 1 [0|1: entry nodes]"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pbrs_amd
from pbrs_amd import scenes, api

sx, sy = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1, 1)  # (a visualiser takes 1 x 1)
sb, cfg = scenes.build_config("c4")
ctx = pbrs_amd.Context(0)
ctx.upload(pbrs_amd.HostScene(sb))
if len(sys.argv) > 3:
    ctx.set_entry_nodes(int(sys.argv[3]))
L = api.gpu_lib()
buf = (C.c_ulonglong * 48)()
ctx.render(sx, sy, cfg["depth"], 1, integrator="normals")
L.pbrs_debug_trav_probe(buf)
img, st = ctx.render(sx, sy, cfg["depth"], 1, timing=True, integrator="normals")
L.pbrs_debug_trav_probe(buf)
print("c4 normals %dx%d spp: ms_extend %.2f ms_raygen %.2f" % (sx, sy, st["ms_extend"], st["ms_raygen"]))
v = [buf[k] for k in range(24)]
rays = max(v[2], 1)
rounds = max(v[0], 1)
print(f"k_extend: {v[2]} rays, {v[0]} wave rounds ({64.0 * v[0] / rays:.1f} lane-rounds per ray), live lanes at round start {v[10] / rounds:.1f}")
print(f"  node steps: first {v[5] / max(v[11], 1):.1f} lanes in {v[11] / rounds:.3f} of rounds, second {v[6] / rounds:.1f}, third {v[7] / rounds:.1f} lanes per round")
print(f"  per ray: node steps {v[16] / rays:.1f}, box tests {v[17] / rays:.1f} (failed {v[18] / rays:.1f}), leaves up {v[19] / rays:.2f} passing {v[20] / rays:.2f}, triangle tests {v[21] / rays:.2f}")
print(f"  boundary steps per ray in {v[22] / rays:.2f} out {v[23] / rays:.2f}")
print("entry_info", ctx.last_entry_info())  # (what the pre-pass found: zeros without the table)
ctx.close()
