"""`ComputeMatches <yaml>` with SIFTmatch.verification_model : 2 -- the homography check, no camera -- writes the rows the Python
matcher computes through the same library, and the same rows with the host twin (MSFM_GEOMETRIC_VERIFICATION=host); an unknown
model is refused."""
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

YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : {mt}
SIFTmatch.verification_model : {model}
"""


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def scene():
    """5 images of a facade: subsets of 600 points of one plane (descriptor per point, slightly perturbed per view) seen through
    synth.scene_cameras, plus rows of their own.  No camera keys: the homography needs none."""
    rng = np.random.default_rng(23)
    n_img, n_pts, n_obs, n_own = 5, 600, 420, 180
    proto = synth.rootsift_images(1, [n_pts + n_img * n_own], seed=23, n_proto=4000)[0]
    cams = synth.scene_cameras(n_img, seed=23, width=W, height=H, focal=FOCAL)
    a, b = rng.uniform(-1.6, 1.6, n_pts), rng.uniform(-1.1, 1.1, n_pts)
    X = np.c_[a, b, 0.25 * a - 0.15 * b]
    descs, kps = [], []
    for i in range(n_img):
        seen = rng.choice(n_pts, n_obs, replace=False)
        d = np.r_[proto[seen], proto[n_pts + i * n_own:n_pts + (i + 1) * n_own]]
        d = np.abs(d + rng.normal(0, 0.003, d.shape).astype(np.float32))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        R, t, f, cx, cy = cams[i]
        k = synth.keypoints(len(d), seed=23 + 100 + i, width=W, height=H)
        Xc = X[seen] @ R.T + t
        k[:n_obs, 0] = (f * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(0, 0.3, n_obs)).astype(np.float32)
        k[:n_obs, 1] = (f * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(0, 0.3, n_obs)).astype(np.float32)
        perm = rng.permutation(len(d))
        descs.append(np.ascontiguousarray(d[perm], np.float32))
        kps.append(np.ascontiguousarray(k[perm]))
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
        cfg.write_text(YAML.format(db=path, mt=mt, model=2))   # (no Reconstruction.Camera.* keys)
        r = run(exe, cfg, env)
        assert r.returncode == 0, r.stderr[-2000:]
    cls = BruteFeatureMatcher if mt == 1 else SequentialFeatureMatcher
    with _lib.Context(0) as ctx:
        cls(b, ctx=ctx, verbose=False, geometric_verification="device", verification_model=2).RunMatching()
    ra, rb, rc = rows(a), rows(b), rows(c)
    assert ra == rb and ra == rc and len(ra) >= 4
    assert sum(r[1] for r in ra) > 200   # the shared points survive the check


def test_unknown_model_exits_non_zero(exe, scene, tmp_path):
    descs, kps = scene
    a = str(tmp_path / "m3.db")
    database.write_synthetic_database(a, descs[:2], kps[:2])
    cfg = tmp_path / "m3.yaml"
    cfg.write_text(YAML.format(db=a, mt=1, model=3))
    r = run(exe, cfg)
    assert r.returncode != 0 and "verification_model" in r.stderr
    assert rows(a) == []
