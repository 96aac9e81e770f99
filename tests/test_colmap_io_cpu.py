"""CPU: the COLMAP scan reader (curve_gaussian_amd.scene.colmap_io) against the reference's own readers
(tests/golden/colmap/, tests/golden/make_colmap_golden.py), its writer, and Scene's dispatch between COLMAP and EMAP."""
import os
import shutil

import numpy as np
import pytest
import torch

from curve_gaussian_amd import synthetic as S
from curve_gaussian_amd.scene import colmap_io as CI
from curve_gaussian_amd.scene import dataset_io as IO

SCAN = os.path.join(os.path.dirname(__file__), "golden", "colmap")
G = np.load(os.path.join(SCAN, "colmap.npz"))
CONFIGS = [str(c) for c in G["configs"]]


def test_binary_and_text_readers_match_the_reference():
    sp = os.path.join(SCAN, "sparse/0")
    for cams in (CI.read_cameras_binary(os.path.join(sp, "cameras.bin")), CI.read_cameras_text(os.path.join(sp, "cameras.txt"))):
        assert sorted(cams) == G["cam_ids"].tolist()
        for k, c in cams.items():
            assert c.model == str(G[f"cam{k}_model"]) and [c.width, c.height] == G[f"cam{k}_wh"].tolist()
            np.testing.assert_array_equal(c.params, G[f"cam{k}_params"])
    for tag, imgs in (("bin", CI.read_images_binary(os.path.join(sp, "images.bin"))),
                      ("txt", CI.read_images_text(os.path.join(sp, "images.txt")))):
        for t in (tag, "bin"):            # the text twin also equals the reference's binary reading
            assert list(imgs) == G[f"img_{t}_ids"].tolist()
            assert [imgs[i].name for i in imgs] == G[f"img_{t}_names"].tolist()
            assert [imgs[i].camera_id for i in imgs] == G[f"img_{t}_camera_ids"].tolist()
            np.testing.assert_array_equal(np.stack([imgs[i].qvec for i in imgs]), G[f"img_{t}_qvec"])
            np.testing.assert_array_equal(np.stack([imgs[i].tvec for i in imgs]), G[f"img_{t}_tvec"])
            np.testing.assert_array_equal(np.concatenate([imgs[i].xys for i in imgs]), G[f"img_{t}_xys"])
            np.testing.assert_array_equal(np.concatenate([imgs[i].point3D_ids for i in imgs]), G[f"img_{t}_p3d"])
    for tag, (xyz, rgb, err) in (("bin", CI.read_points3D_binary(os.path.join(sp, "points3D.bin"))),
                                 ("txt", CI.read_points3D_text(os.path.join(sp, "points3D.txt")))):
        np.testing.assert_array_equal(xyz, G[f"p3d_{tag}_xyz"])
        np.testing.assert_array_equal(rgb, G[f"p3d_{tag}_rgb"])
        np.testing.assert_array_equal(err, G[f"p3d_{tag}_err"])


def _check_config(key, train, test, extent):
    assert [c.image_name for c in train] == G[key + "_train"].tolist()
    assert [c.image_name for c in test] == G[key + "_test"].tolist()
    assert [c.image_name in G[key + "_test"].tolist() for c in train] == G[key + "_is_test"].tolist()
    assert [c.uid for c in train] == G[key + "_uid"].tolist()
    np.testing.assert_array_equal(np.stack([c.R for c in train]), G[key + "_R"])
    np.testing.assert_array_equal(np.stack([c.T for c in train]), G[key + "_T"])
    np.testing.assert_array_equal([c.FoVx for c in train], G[key + "_fovx"])
    np.testing.assert_array_equal([c.FoVy for c in train], G[key + "_fovy"])
    K, Kref = np.stack([c.K for c in train]), G[key + "_K"]
    simple = np.array([c.FoVx != c.FoVy and c.K[0, 0] == c.K[1, 1] for c in train])   # SIMPLE_PINHOLE: f on both axes
    np.testing.assert_array_equal(K[~simple], Kref[~simple])
    np.testing.assert_array_equal(K[simple][:, 0], Kref[simple][:, 0])                # (the reference's fy is stale there)
    assert extent == float(G[key + "_extent"])


@pytest.mark.parametrize("key", CONFIGS)
def test_read_colmap_matches_read_colmap_scene_info(key):
    det, ev, hold = key.split("_")
    train, test, pcd, extent = CI.read_colmap(SCAN, eval=bool(int(ev)), llffhold=int(hold), detector=det)
    _check_config(key, train, test, extent)
    assert len(train) == 10 and set(map(id, test)) <= set(map(id, train))                  # train keeps the test cameras
    # points3D.ply is present: fetchPly's positions, colours / 255 and normals
    np.testing.assert_array_equal(pcd.points, G["ply_points"])
    np.testing.assert_array_equal(pcd.colors, G["ply_colors"])
    np.testing.assert_array_equal(pcd.normals, G["ply_normals"])


def test_jpg_names_are_never_test_cameras():
    train, test, _, _ = CI.read_colmap(SCAN, eval=True, llffhold=1)
    assert {c.image_name for c in test} == {c.image_name for c in train} - {"frame_001.png", "frame_004.png", "frame_006.png"}


@pytest.mark.parametrize("det", ["DexiNed", "PidiNet"])
@pytest.mark.parametrize("res", [-1, 2])
def test_loaded_images_and_cameras_match_load_cam(det, res):
    train, _, _, _ = CI.read_colmap(SCAN, eval=True, detector=det, resolution=res)
    chans = set()
    for i, c in enumerate(train):
        k = f"{det}_r{res}_{i}"
        np.testing.assert_array_equal(c.original_image.numpy(), G[k + "_image"])
        np.testing.assert_array_equal(c.world_view_transform.numpy(), G[k + "_wv"])
        np.testing.assert_array_equal(c.full_proj_transform.numpy(), G[k + "_full"])
        np.testing.assert_array_equal(c.camera_center.numpy(), G[k + "_center"])
        assert (c.image_height, c.image_width) == c.original_image.shape[1:]
        chans.add(c.original_image.shape[0])
    assert chans == {1, 3}
    widths = sorted(c.image_width for c in train)
    assert widths[-1] == (1600 if res == -1 else 850)                                      # the 1700 px image


def test_text_twin_reads_like_the_binary_model(tmp_path):
    scan = str(tmp_path / "scan")
    shutil.copytree(SCAN, scan)
    for f in ("cameras.bin", "images.bin", "points3D.bin", "points3D.ply"):
        os.remove(os.path.join(scan, "sparse/0", f))
    train, test, pcd, extent = CI.read_colmap(scan, eval=True, llffhold=3)
    _check_config("DexiNed_1_3", train, test, extent)
    # without points3D.ply the cloud comes from points3D.bin / .txt (deviation: the reference's cloud is None)
    np.testing.assert_array_equal(pcd.points, G["p3d_txt_xyz"])
    np.testing.assert_array_equal(pcd.colors, G["p3d_txt_rgb"] / 255.0)
    assert not pcd.normals.any()


def test_llffhold_zero_reads_test_txt():
    _, test, _, _ = CI.read_colmap(SCAN, eval=True, llffhold=0)
    assert [c.image_name for c in test] == ["frame_002.png", "frame_007.png"]               # frame_001.jpg never matches


def test_unknown_camera_model_raises(tmp_path):
    scan = str(tmp_path / "scan")
    shutil.copytree(SCAN, scan)
    sp = os.path.join(scan, "sparse/0")
    cams = CI.read_cameras_binary(os.path.join(sp, "cameras.bin"))
    cams[2] = CI.ColmapCamera(2, "SIMPLE_RADIAL", 48, 32, np.array([40.0, 24.0, 16.0, 0.01]))
    CI.write_cameras_binary(os.path.join(sp, "cameras.bin"), cams)
    with pytest.raises(ValueError, match="SIMPLE_RADIAL not handled"):
        CI.read_colmap(scan)


def test_write_colmap_round_trip(tmp_path):
    cams = S.room_cameras(5, 24, 40, 4)
    g = torch.Generator().manual_seed(1)
    maps = [(torch.rand(1, 24, 40, generator=g) * 255).round() / 255 for _ in cams]
    pts = np.random.default_rng(0).normal(size=(30, 3))
    for binary in (True, False):
        scan = str(tmp_path / f"scan{int(binary)}")
        CI.write_colmap(scan, cams, maps, pts, binary=binary)
        train, test, pcd, extent = CI.read_colmap(scan, eval=True, llffhold=2)
        assert [c.image_name for c in train] == [f"{i:05d}.png" for i in range(5)]
        assert [c.image_name for c in test] == ["00000.png", "00002.png", "00004.png"]
        for a, b, m in zip(cams, train, maps):
            np.testing.assert_allclose(b.full_proj_transform.numpy(), a.full_proj_transform.numpy(), atol=1e-5)
            np.testing.assert_allclose(b.camera_center.numpy(), a.camera_center.numpy(), atol=1e-5)
            assert b.FoVx == pytest.approx(a.FoVx, rel=1e-12) and b.FoVy == pytest.approx(a.FoVy, rel=1e-12)
            np.testing.assert_allclose(b.original_image.numpy(), m.numpy(), atol=1e-7)
        np.testing.assert_allclose(pcd.points, pts, rtol=1e-15)
        centres = np.stack([c.camera_center.numpy() for c in cams]).astype(np.float64)
        assert extent == pytest.approx(1.1 * np.linalg.norm(centres - centres.mean(0), axis=1).max(), rel=1e-5)


def test_ply_table_reads_ascii_and_uchar_colours(tmp_path):
    p = str(tmp_path / "a.ply")
    with open(p, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment x\nelement vertex 2\nproperty double x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 0\n"
                "property list uchar int vertex_indices\nend_header\n0.5 1 2 255 0 7\n-1.25 3 4 1 2 3\n")
    v = IO.read_ply_table(p)
    np.testing.assert_array_equal(v["x"], [0.5, -1.25])
    assert v["red"].dtype == np.uint8 and v["blue"].tolist() == [7, 3]
    # the float32 tables save_ply writes read the same through both readers
    q = str(tmp_path / "b.ply")
    with open(q, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nend_header\n")
        f.write(np.arange(6, dtype="<f4").tobytes())
    a, b = IO.read_ply_table(q), IO.read_ply_vertices(q)
    assert all((a[k] == b[k]).all() for k in ("x", "y"))


def test_scene_dispatch_keeps_emap_scans_as_they_are(tmp_path):
    """Scene on an EMAP scan reads the cameras read_emap reads (today's path); eval=True gives the same frames as the test
    list; a COLMAP scan goes through read_colmap.  create_from_pcd is recorded, not run (it needs the GPU)."""
    from curve_gaussian_amd.scene.gaussian_curve_model import Scene

    class Rec:
        def create_from_pcd(self, pcd, cams, extent):
            self.args = (pcd, cams, extent)

    cams = S.fibonacci_cameras(3, 16, 16)
    IO.write_emap(str(tmp_path / "emap"), cams, [torch.zeros(1, 16, 16)] * 3)
    ref = IO.read_emap(str(tmp_path / "emap"))
    for ev in (False, True):
        r = Rec()
        sc = Scene(str(tmp_path / "emap"), r, rng=np.random.default_rng(0), eval=ev)
        assert [c.image_name for c in sc.getTrainCameras()] == [c.image_name for c in ref]
        for a, b in zip(sc.getTrainCameras(), ref):
            assert torch.equal(a.full_proj_transform, b.full_proj_transform) and torch.equal(a.original_image, b.original_image)
        assert sc.getTestCameras() == (sc.getTrainCameras() if ev else [])
        assert r.args[0].points.shape == (3375, 3) and r.args[1] is sc.train_cameras
    r = Rec()
    sc = Scene(SCAN, r, eval=True)
    assert [c.image_name for c in sc.getTrainCameras()] == G["DexiNed_1_8_train"].tolist()
    assert [c.image_name for c in sc.getTestCameras()] == G["DexiNed_1_8_test"].tolist()
    assert sc.cameras_extent == float(G["DexiNed_1_8_extent"]) and r.args[0].points.shape == (25, 3)
