"""`ComputeMatches <yaml>` with SIFTmatch.two_view_geometry : 1 (under verification_model : 1) on a synth.south_building_database:
the matches table is byte-identical to the run with the key off; two_view_geometries has one row per matches row the verification
wrote, equal to the Python binding's records; a killed and resumed run ends with the same two tables; the device and the host-RANSAC
executables write the same table; the key without verification_model : 1 exits non-zero with its message."""
import os
import re
import shutil
import signal
import subprocess

import numpy as np
import pytest

from monocularsfm_amd import _lib, database, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
EXE = os.path.join(HOST, "ComputeMatches")
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : 1
SIFTmatch.verification_model : {model}
SIFTmatch.two_view_geometry : {tv}
Reconstruction.Camera.fx: 2500.0
Reconstruction.Camera.fy: 2500.0
Reconstruction.Camera.cx: 1536.0
Reconstruction.Camera.cy: 1152.0
Reconstruction.Camera.k1: 0.0
Reconstruction.Camera.k2: 0.0
Reconstruction.Camera.p1: 0.0
Reconstruction.Camera.p2: 0.0
{extra}"""
COLS = ("pair_id, valid, n_kept, n_positive_depth, n_triangulated, is_initial_candidate, median_tri_angle, mean_tri_angle, "
        "mean_residual, pose")
N_IMG = 24


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tv") / "base.db")
    descs, kps = synth.south_building_database(path, N_IMG, 500, seed=91)
    return path, descs, kps


def copy_db(src, dst):
    shutil.copy(src, dst)
    for ext in ("-wal", "-shm"):
        if os.path.exists(src + ext):
            shutil.copy(src + ext, dst + ext)
    return dst


def tables(path):
    db = database.Database(path)
    m = db.db.execute("SELECT pair_id, rows, cols, data FROM matches ORDER BY pair_id").fetchall()
    has = db.db.execute("SELECT count(*) FROM sqlite_master WHERE name = 'two_view_geometries'").fetchone()[0]
    g = db.db.execute("SELECT %s FROM two_view_geometries ORDER BY pair_id" % COLS).fetchall() if has else None
    db.Close()
    return m, g


def run(exe, tmp_path, db, tv, model=1, env_extra=None, extra=""):
    cfg = tmp_path / (os.path.basename(db) + ".yaml")
    cfg.write_text(YAML.format(db=db, model=model, tv=tv, extra=extra))
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=env, timeout=600), cfg, env


def test_table_equals_the_binding_and_matches_do_not_change(exe, base, tmp_path):
    src, descs, kps = base
    off, on = copy_db(src, str(tmp_path / "off.db")), copy_db(src, str(tmp_path / "on.db"))
    r_off, _, _ = run(exe, tmp_path, off, 0)
    # (pairs of 500-row images keep fewer than the default 100 matches: the optional key lowers the bar so both verdicts occur)
    r_on, _, _ = run(exe, tmp_path, on, 1, extra="SIFTmatch.two_view_min_num_inliers : 20\n")
    assert r_off.returncode == 0 and r_on.returncode == 0, (r_off.stderr[-1000:], r_on.stderr[-1000:])
    assert r_on.stdout.split("Elapsed")[0] == r_off.stdout.split("Elapsed")[0]
    strip = lambda s: re.sub(r"\t .*seconds.*\n|.*minutes.*\n|.*\[msfm.*\n", "", s)   # noqa: E731  (the timing lines)
    assert strip(r_on.stdout) == strip(r_off.stdout)
    m_off, g_off = tables(off)
    m_on, g_on = tables(on)
    assert g_off is None and m_on == m_off and len(m_on) > 100
    assert [r[0] for r in g_on] == [r[0] for r in m_on]        # one row per matches row
    # the binding's records of the same pairs, in the executable's orientation (stdout: "Compute Matches a - b ...")
    pairs = [(int(a), int(b)) for a, b in re.findall(r"Compute Matches (\d+) - (\d+) \.\.\.", r_on.stdout)]
    assert len(pairs) == len(m_on)
    db = database.Database(on)
    ids = [r[0] for r in db.db.execute("SELECT image_id FROM images ORDER BY image_id")]
    db.Close()
    with _lib.Context(0) as ctx:
        for i, d, k in zip(ids, descs, kps):
            ctx.upload_image(i, d)
            ctx.upload_keypoints(i, k)
        ctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
        ctx.set_two_view_geometry(True, min_num_inliers=20)
        offs, qt, _ = ctx.match_pairs_verified(np.asarray(pairs, np.int32), ratio=0.8, cross_check=True, max_distance=0.7)
        rec = ctx.two_view_geometry(len(pairs))
    got = dict((r[0], r[1:]) for r in g_on)
    n_by_pair = dict((r[0], r[1]) for r in m_on)
    assert int(rec["valid"].sum()) > 50 and rec["is_initial_candidate"].any()
    for p, (a, b) in enumerate(pairs):
        pid = _lib.pair_id(a, b) if hasattr(_lib, "pair_id") else database.Database.ImagePairToPairId(a, b)
        assert n_by_pair[pid] == offs[p + 1] - offs[p]
        r = rec[p]
        want = (int(r["valid"]), int(r["n_kept"]), int(r["n_positive_depth"]), int(r["n_triangulated"]), int(r["is_initial_candidate"]),
                float(r["median_tri_angle"]), float(r["mean_tri_angle"]), float(r["mean_residual"]))
        assert tuple(got[pid][:8]) == want
        assert bytes(got[pid][8]) == r["R"].astype("<f8").tobytes() + r["t"].astype("<f8").tobytes() and len(got[pid][8]) == 96


def test_host_ransac_executable_writes_the_same_table(exe, base, tmp_path):
    src, _, _ = base
    dev, host = copy_db(src, str(tmp_path / "dev.db")), copy_db(src, str(tmp_path / "host.db"))
    r1, _, _ = run(exe, tmp_path, dev, 1)
    r2, _, _ = run(exe, tmp_path, host, 1, env_extra={"MSFM_GEOMETRIC_VERIFICATION": "host"})
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-1000:])
    assert tables(dev) == tables(host) and len(tables(dev)[1]) > 100


def test_with_model_selection_both_executables(exe, base, tmp_path):
    src, _, _ = base
    dev, host = copy_db(src, str(tmp_path / "dev.db")), copy_db(src, str(tmp_path / "host.db"))
    r1, _, _ = run(exe, tmp_path, dev, 1, extra="SIFTmatch.model_selection : 1\n")
    r2, _, _ = run(exe, tmp_path, host, 1, env_extra={"MSFM_GEOMETRIC_VERIFICATION": "host"}, extra="SIFTmatch.model_selection : 1\n")
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-1000:])
    assert tables(dev) == tables(host)


def test_killed_and_resumed_run_ends_with_the_same_tables(exe, base, tmp_path):
    src, _, _ = base
    clean, cut = copy_db(src, str(tmp_path / "clean.db")), copy_db(src, str(tmp_path / "cut.db"))
    r, _, _ = run(exe, tmp_path, clean, 1)
    assert r.returncode == 0, r.stderr[-1000:]
    want_m, want_g = tables(clean)
    cfg = tmp_path / "cut.db.yaml"
    cfg.write_text(YAML.format(db=cut, model=1, tv=1, extra=""))
    p = subprocess.Popen([exe, str(cfg)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    seen = 0
    for line in p.stdout:
        if line.startswith("Compute Matches"):
            seen += 1
            if seen >= len(want_m) // 3:
                break
    p.send_signal(signal.SIGKILL)
    p.stdout.close()
    p.wait()
    part_m, part_g = tables(cut)
    assert 0 < len(part_m) < len(want_m)
    assert part_g is not None and [r[0] for r in part_g] == [r[0] for r in part_m]   # the two rows of a pair share a transaction
    assert set(part_m) <= set(want_m) and set(part_g) <= set(want_g)
    r, _, _ = run(exe, tmp_path, cut, 1)
    assert r.returncode == 0 and r.stdout.count("Existing, Continue!") == len(part_m)
    assert tables(cut) == (want_m, want_g)


@pytest.mark.parametrize("model", [0, 2])
def test_key_without_the_essential_model_exits_non_zero(exe, base, tmp_path, model):
    src, _, _ = base
    db = copy_db(src, str(tmp_path / "bad.db"))
    r, _, _ = run(exe, tmp_path, db, 1, model=model)
    assert r.returncode != 0 and "SIFTmatch.two_view_geometry" in r.stderr and "verification_model : 1" in r.stderr
    assert tables(db) == ([], None)
    for extra in ("SIFTmatch.two_view_tri_max_error : -1.0\n", "SIFTmatch.two_view_min_num_inliers : -3\n"):
        r, _, _ = run(exe, tmp_path, db, 1, extra=extra)
        assert r.returncode != 0 and "two_view" in r.stderr
