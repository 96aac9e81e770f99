"""Emits tests/golden/edge_clip_parent.json: what the depth-gated tools and ``ChunkDepth.settings()`` write WITHOUT near-plane
clipping, recorded by the commit before ``near_clip`` existed, so that tests/test_edge_clip_cpu.py can hold the option's
absence to them (settings byte for byte, keys in their order, numbers as parsed).  Data only (JSON texts); host back end, no GPU.  ``recordings`` is shared with the test, which calls
it on the current code.
usage: python tests/golden/make_edge_clip_golden.py        (on the commit whose bytes are to be recorded)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DST = os.path.join(HERE, "edge_clip_parent.json")


def recordings(work_dir):
    """name -> text.  Everything is written below ``work_dir`` with RELATIVE paths (the cwd is changed for the calls and
    restored), so the recorded settings hold no absolute path."""
    import numpy as np
    from curve_gaussian_amd.edge_extraction import reprojection as R
    from curve_gaussian_amd.edge_extraction import support as SUP
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.scene import solid_scan as SS
    out = {}
    cwd = os.getcwd()
    os.chdir(work_dir)
    try:
        scan = SS.solid_scan("box", 3, 24, 32, backend="host")
        SS.write_solid_scan(os.path.join("data", "box"), scan, depth=True)
        os.makedirs(os.path.join("out", "box"), exist_ok=True)
        with open(os.path.join("out", "box", "parametric_edges.json"), "w") as f:
            json.dump(scan.edges, f)
        for name, kw in (("tris", dict(occluder=scan.tris)), ("path", dict(occluder=os.path.join("data", "box", "mesh.ply"))),
                         ("maps", dict(depth_maps=list(scan.depth))), ("none", {})):
            out["settings_" + name] = json.dumps(EO.ChunkDepth("x", scan.cameras, **kw).settings())
        res = R.score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend="host", occluder=scan.tris)
        out["score_edges"] = json.dumps(res)
        common = ["--base_dir", "out", "--dataset_dir", "data", "--detector", "PidiNet", "--backend", "host"]
        for flags, tag in ((["--occluder", "mesh.ply"], "occluder"), (["--depth_dir", "depth"], "depth_dir"), ([], "plain")):
            R.main(common + flags)
            out["reprojection_" + tag] = open(os.path.join("out", "box", R.SCORE_FILE)).read()
            SUP.main(common + flags + ["--tolerances", "1", "2", "--keep_tolerance", "1", "--snap", "--snap_iterations", "1",
                                       "--trim"])
            for n in (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE):
                out[f"{n}_{tag}"] = open(os.path.join("out", "box", n)).read()
        from curve_gaussian_amd.ops import edge_seed as SD
        _, info = SD.seed_points(scan.cameras, scan.maps, "PidiNet", ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), grid=16,
                                 backend="host", occluder=scan.tris)
        out["seed_info"] = json.dumps(info, default=lambda o: np.asarray(o).tolist())
    finally:
        os.chdir(cwd)
    return out


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with tempfile.TemporaryDirectory() as d:
        rec = recordings(d)
    with open(DST, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", DST, len(rec), "recordings,", os.path.getsize(DST), "bytes")
