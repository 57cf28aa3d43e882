"""Build-time probe of the node octree at scale (not a test): the reference's box surface (46 786 triangles)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import wtp_amd as w

z = np.load(os.path.join(ROOT, "tests", "golden", "box_mesh.npz"))
for dt in (np.float32, np.float64):
    v, t = z["vertices"].astype(dt), z["triangles"].astype(np.int32)
    with w.Context(0) as ctx:
        ctx.mesh_set(v, t)
        for h in (0.8, 0.4, 0.2, 0.1):
            for rep in range(2):
                t0 = time.perf_counter()
                info = ctx.node_tree_build(h, 2.0, 1e-6)
                dtm = time.perf_counter() - t0
            t0 = time.perf_counter()
            got = ctx.node_tree_get(info["n_leaves"], want=("cls",))
            tg = time.perf_counter() - t0
            pts = (np.random.default_rng(0).random((1_000_000, 3)) * 25).astype(dt)
            t0 = time.perf_counter()
            leaf = ctx.node_tree_locate(pts)
            tl = time.perf_counter() - t0
            print(f"{np.dtype(dt).name} h={h}: leaves={info['n_leaves']} int/bnd/ext={info['n_interior']}/{info['n_boundary']}/{info['n_exterior']} "
                  f"depth={info['depth_max']} rounds={info['balance_rounds']} syncs={info['host_syncs']} auto={info['max_points_auto']} "
                  f"build={dtm*1e3:.1f} ms get={tg*1e3:.1f} ms locate(1e6)={tl*1e3:.1f} ms inroot={(leaf>=0).mean():.3f}", flush=True)
        law = w.sampling._sampler_spacing(w.BoundaryLayerSpacing(v[::50].astype(dt), 0.1, 1.0, 2.0))
        t0 = time.perf_counter()
        info = ctx.node_tree_build(law, 2.0, 1e-6)
        print(f"{np.dtype(dt).name} BL 0.1->1.0 over 2.0: leaves={info['n_leaves']} depth={info['depth_max']} rounds={info['balance_rounds']} "
              f"build={(time.perf_counter()-t0)*1e3:.1f} ms", flush=True)
