"""`ComputeMatches <yaml>` with SIFTmatch.verification_model : 1 -- the essential-matrix check with the camera of
Reconstruction.Camera.* -- writes the rows the Python matcher computes through the same library, and the same rows with the host
twin (MSFM_GEOMETRIC_VERIFICATION=host); a configuration without the camera is refused."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from monocularsfm_amd import _lib, database, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
EXE = os.path.join(HOST, "ComputeMatches")
W, H, FOCAL = 3072, 2304, 2500.0
DIST = (-0.08, 0.02, 2e-4, -1e-4)

YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : {mt}
SIFTmatch.verification_model : 1
{camera}
"""
CAMERA = """Reconstruction.Camera.fx: 2500.0
Reconstruction.Camera.fy: 2500.0
Reconstruction.Camera.cx: 1536.0
Reconstruction.Camera.cy: 1152.0
Reconstruction.Camera.k1: -0.08
Reconstruction.Camera.k2: 0.02
Reconstruction.Camera.p1: 0.0002
Reconstruction.Camera.p2: -0.0001"""


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def scene():
    """5 images observing subsets of 600 shared 3-D points (descriptor per point, slightly perturbed per view) through
    synth.scene_cameras and a distorting lens, plus rows of their own."""
    rng = np.random.default_rng(17)
    n_img, n_pts, n_obs, n_own = 5, 600, 420, 180
    proto = synth.rootsift_images(1, [n_pts + n_img * n_own], seed=17, n_proto=4000)[0]
    cams = synth.scene_cameras(n_img, seed=17, width=W, height=H, focal=FOCAL)
    ids, descs = [], []
    for i in range(n_img):
        seen = rng.choice(n_pts, n_obs, replace=False)
        d = np.r_[proto[seen], proto[n_pts + i * n_own:n_pts + (i + 1) * n_own]]
        d = np.abs(d + rng.normal(0, 0.003, d.shape).astype(np.float32))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        perm = rng.permutation(len(d))
        ids.append(np.r_[seen, np.full(n_own, -1)][perm])
        descs.append(np.ascontiguousarray(d[perm], np.float32))
    kps = synth.scene_keypoints(ids, cams, n_pts, seed=17, noise_px=0.5)
    k1, k2, p1, p2 = DIST
    for k in kps:
        x = (k[:, 0].astype(np.float64) - W / 2) / FOCAL
        y = (k[:, 1].astype(np.float64) - H / 2) / FOCAL
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 * r2
        k[:, 0] = (FOCAL * (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + W / 2).astype(np.float32)
        k[:, 1] = (FOCAL * (y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + H / 2).astype(np.float32)
    return descs, kps


def rows(path):
    db = database.Database(path)
    r = db.db.execute("SELECT pair_id, rows, cols, data FROM matches ORDER BY pair_id").fetchall()
    db.Close()
    return r


def run(exe, cfg, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("mt", [0, 1])
def test_cli_rows_equal_python_and_the_host_twin(exe, scene, tmp_path, mt):
    from monocularsfm_amd.matcher import BruteFeatureMatcher, SequentialFeatureMatcher
    descs, kps = scene
    a, b, c = str(tmp_path / "cli.db"), str(tmp_path / "py.db"), str(tmp_path / "host.db")
    database.write_synthetic_database(a, descs, kps)
    shutil.copy(a, b)
    shutil.copy(a, c)
    for path, env in ((a, {}), (c, {"MSFM_GEOMETRIC_VERIFICATION": "host"})):
        cfg = tmp_path / (os.path.basename(path) + ".yaml")
        cfg.write_text(YAML.format(db=path, mt=mt, camera=CAMERA))
        r = run(exe, cfg, env)
        assert r.returncode == 0, r.stderr[-2000:]
    cls = BruteFeatureMatcher if mt == 1 else SequentialFeatureMatcher
    cam = (FOCAL, FOCAL, W / 2, H / 2) + DIST
    with _lib.Context(0) as ctx:
        cls(b, ctx=ctx, verbose=False, geometric_verification="device", verification_model=1, camera=cam).RunMatching()
    ra, rb, rc = rows(a), rows(b), rows(c)
    assert ra == rb and ra == rc and len(ra) >= 4
    assert sum(r[1] for r in ra) > 200   # the shared points survive the check


def test_missing_camera_exits_non_zero(exe, scene, tmp_path):
    descs, kps = scene
    a = str(tmp_path / "nocam.db")
    database.write_synthetic_database(a, descs[:2], kps[:2])
    cam_without_cy = "\n".join(l for l in CAMERA.splitlines() if ".cy" not in l)
    for camera in ("", cam_without_cy):
        cfg = tmp_path / "nocam.yaml"
        cfg.write_text(YAML.format(db=a, mt=1, camera=camera))
        r = run(exe, cfg)
        assert r.returncode != 0 and "Reconstruction.Camera" in r.stderr
    assert rows(a) == []
