"""`ComputeMatches <yaml>` with SIFTmatch.triangulation : 1 on a synth.south_building_database whose cameras are known: the `points3D`
table equals Context.points3d() for the same job (the run's `matches` rows folded through tracks_add, the same poses, camera and
parameters), value for value; with the key the `matches` and `tracks` tables and stdout are what they are without it, and without it
there is no `points3D` table; bad poses files and missing keys exit non-zero before anything is matched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from monocularsfm_amd import _lib, database, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
EXE = os.path.join(HOST, "ComputeMatches")
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAMERA = "".join("Reconstruction.Camera.%s : %r\n" % kv for kv in zip(("fx", "fy", "cx", "cy"), CAM))
YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : 1
{extra}"""
N_IMG, SEED = 24, 91
UNPOSED = (5, 17)


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    d = tmp_path_factory.mktemp("triangulation")
    path = str(d / "base.db")
    descs, kps = synth.south_building_database(path, N_IMG, 500, seed=SEED)
    cams = synth.scene_cameras(N_IMG, seed=SEED + 7)
    poses = {i: (cams[i][0], cams[i][1]) for i in range(N_IMG) if i not in UNPOSED}
    pf = d / "poses.txt"
    lines = ["# image_id r00 .. r22 tx ty tz"]
    for i in sorted(poses, reverse=True):                          # (any order)
        lines.append(" ".join([str(i)] + [repr(float(v)) for v in np.r_[poses[i][0].reshape(9), poses[i][1]]]) + ("   # a comment" if i % 2 else ""))
    pf.write_text("\n".join(lines) + "\n\n")
    return path, descs, kps, poses, str(pf)


def copy_db(src, dst):
    shutil.copy(src, dst)
    for ext in ("-wal", "-shm"):
        if os.path.exists(src + ext):
            shutil.copy(src + ext, dst + ext)
    return dst


def run(exe, tmp_path, db, extra, expect_ok=True):
    cfg = tmp_path / (os.path.basename(db) + ".yaml")
    cfg.write_text(YAML.format(db=db, extra=extra))
    r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=dict(os.environ, MSFM_CLI_TIMING="1"), timeout=600)
    if expect_ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def tables(path):
    db = database.Database(path)
    out = {}
    for name, cols in (("matches", "pair_id, rows, cols, data"), ("tracks", "track_id, length, consistent, elements"),
                       ("points3D", "track_id, status, n_views, x, y, z, mean_residual, tri_angle, residuals")):
        has = db.db.execute("SELECT count(*) FROM sqlite_master WHERE name = ?", (name,)).fetchone()[0]
        out[name] = db.db.execute("SELECT %s FROM %s ORDER BY 1" % (cols, name)).fetchall() if has else None
    db.Close()
    return out


def whole(path, without=()):
    """Everything the database file holds: the schema (sqlite_master, in order) and every row of every table, blobs as bytes."""
    db = database.Database(path)
    master = [r for r in db.db.execute("SELECT type, name, tbl_name, sql FROM sqlite_master ORDER BY rowid") if r[2] not in without]
    rows = {name: db.db.execute("SELECT * FROM \"%s\" ORDER BY 1" % name).fetchall() for kind, name, _, _ in master if kind == "table"}
    db.Close()
    return master, rows


def strip(s):
    return re.sub(r"\t .*seconds.*\n|.*minutes.*\n|.*\[msfm.*\n|Elapsed.*\n", "", s)   # (the timing lines)


def library_points(base, matches, params=(2.0, 1.5, 2), min_pair=10):
    """The same job through the library: the stored rows folded with tracks_add, the same poses -> (tracks, points, residuals)"""
    _, descs, kps, poses, _ = base
    pairs = np.asarray([(pid // 10000, pid % 10000) for pid, _, _, _ in matches], np.int32).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum([r for _, r, _, _ in matches])]).astype(np.int64)
    qt = np.concatenate([np.frombuffer(d or b"", "<i4").reshape(-1, 2) for _, _, _, d in matches] + [np.zeros((0, 2), np.int32)])
    with _lib.Context(0) as ctx:
        for i in range(N_IMG):
            ctx.upload_image(i, descs[i])
            ctx.upload_keypoints(i, kps[i])
        ctx.tracks_begin(np.arange(N_IMG, dtype=np.int32), min_pair_matches=min_pair, add_only=True)
        ctx.tracks_add(pairs, offsets, qt)
        ctx.tracks_finish()
        tracks = ctx.tracks()
        ctx.triangulate_tracks(CAM, poses, *params)
        pts, res = ctx.points3d()
        ctx.tracks_end()
    return tracks, pts, res


def check_points(rows, tracks, pts, res):
    assert rows is not None and len(rows) == len(pts)
    o = tracks[0]
    for t, (track_id, status, n_views, x, y, z, mean, angle, blob) in enumerate(rows):
        p = pts[t]
        assert track_id == t and status == int(p["status"]) and n_views == int(p["n_views"])
        got = np.asarray([x, y, z, np.nan if mean is None else mean, angle], np.float64)
        want = np.r_[p["X"], p["mean_residual"], p["tri_angle"]]
        assert got.tobytes() == want.tobytes() or (np.isnan(got[3]) and np.isnan(want[3]) and np.array_equal(np.delete(got, 3), np.delete(want, 3))), t
        assert np.frombuffer(blob, "<f8").tobytes() == res[o[t]:o[t + 1]].tobytes(), t


def test_points3d_table_equals_the_library(exe, base, tmp_path):
    off = copy_db(base[0], str(tmp_path / "off.db"))
    on = copy_db(base[0], str(tmp_path / "on.db"))
    r_off = run(exe, tmp_path, off, "SIFTmatch.tracks : 1\n" + CAMERA)
    r_on = run(exe, tmp_path, on, "SIFTmatch.tracks : 1\nSIFTmatch.triangulation : 1\nSIFTmatch.triangulation_poses : \"%s\"\n" % base[4] + CAMERA)
    t_off, t_on = tables(off), tables(on)
    # without the key: no points3D table; with it: matches, tracks and stdout are what they are without it
    assert t_off["points3D"] is None and len(t_off["matches"]) > 100 and len(t_off["tracks"]) > 50
    assert t_on["matches"] == t_off["matches"] and t_on["tracks"] == t_off["tracks"] and strip(r_on.stdout) == strip(r_off.stdout)
    assert len(re.findall(r"^\[msfm triangulation\] ", r_on.stderr, re.M)) == 1 and "[msfm triangulation]" not in r_off.stderr
    # ... literally: the same schema objects in the same order and the same rows in every table, but for points3D; and a second run
    # without the key on a fresh copy gives the same file content again (the key leaves no trace when it is off)
    assert whole(on, without=("points3D",)) == whole(off) and all(r[2] != "points3D" for r in whole(off)[0])
    off2 = copy_db(base[0], str(tmp_path / "off2.db"))
    run(exe, tmp_path, off2, "SIFTmatch.tracks : 1\n")              # (no camera keys either: nothing reads them)
    assert whole(off2) == whole(off)
    tracks, pts, res = library_points(base, t_on["matches"])
    check_points(t_on["points3D"], tracks, pts, res)
    ok = _lib.succeeded(pts)
    assert ok.sum() > 30 and (pts["status"] == 0).sum() > 0 and (res == -1.0).sum() > 0      # (the unposed images leave their marks)
    for (tid, length, _, elements), row in zip(t_on["tracks"], t_on["points3D"]):
        assert len(row[8]) == 8 * length and tid == row[0]


def test_parameter_keys_under_the_essential_matrix_model(exe, base, tmp_path):
    """The optional keys reach the library; the essential-matrix model and the triangulation share the camera keys."""
    db = copy_db(base[0], str(tmp_path / "p.db"))
    run(exe, tmp_path, db, "SIFTmatch.tracks : 1\nSIFTmatch.tracks_min_num_matches : 25\nSIFTmatch.verification_model : 1\n"
                           "SIFTmatch.triangulation : 1\nSIFTmatch.triangulation_poses : \"%s\"\nSIFTmatch.triangulation_max_error : 1.0\n"
                           "SIFTmatch.triangulation_min_angle : 4.0\nSIFTmatch.triangulation_min_views : 3\n" % base[4] + CAMERA)
    t = tables(db)
    tracks, pts, res = library_points(base, t["matches"], (1.0, 4.0, 3), min_pair=25)
    check_points(t["points3D"], tracks, pts, res)
    assert (pts["status"] == 0).sum() > 0 and _lib.succeeded(pts).sum() > 10


def test_bad_poses_files_and_missing_keys_exit_before_matching(exe, base, tmp_path):
    good = open(base[4]).read()
    first = [l for l in good.split("\n") if l and not l.startswith("#")][0].split("#")[0].split()
    cases = {
        "twelve": " ".join(first[:12]) + "\n",
        "fourteen": " ".join(first + ["1.0"]) + "\n",
        "word": " ".join(first[:5] + ["abc"] + first[6:]) + "\n",
        "nan": " ".join(first[:5] + ["nan"] + first[6:]) + "\n",
        "twice": " ".join(first) + "\n" + " ".join(first) + "\n",
        "fraction": " ".join(["1.5"] + first[1:]) + "\n",
        "negative": " ".join(["-1"] + first[1:]) + "\n",
        "beyond": " ".join([str(N_IMG)] + first[1:]) + "\n",          # an image the database does not hold
    }
    key = "SIFTmatch.tracks : 1\nSIFTmatch.triangulation : 1\n"
    configs = {name: key + "SIFTmatch.triangulation_poses : \"%s\"\n" % str(tmp_path / (name + ".txt")) + CAMERA for name in cases}
    for name, text in cases.items():
        (tmp_path / (name + ".txt")).write_text(text)
    configs["no-file"] = key + "SIFTmatch.triangulation_poses : \"%s\"\n" % str(tmp_path / "absent.txt") + CAMERA
    configs["no-poses-key"] = key + CAMERA
    configs["no-camera"] = key + "SIFTmatch.triangulation_poses : \"%s\"\n" % base[4]
    configs["no-tracks"] = "SIFTmatch.triangulation : 1\nSIFTmatch.triangulation_poses : \"%s\"\n" % base[4] + CAMERA
    configs["bad-switch"] = "SIFTmatch.tracks : 1\nSIFTmatch.triangulation : 2\n" + CAMERA
    configs["negative-error"] = key + "SIFTmatch.triangulation_poses : \"%s\"\nSIFTmatch.triangulation_max_error : -1.0\n" % base[4] + CAMERA
    for name, extra in configs.items():
        db = copy_db(base[0], str(tmp_path / (name + ".db")))
        r = run(exe, tmp_path, db, extra, expect_ok=False)
        assert r.returncode != 0 and r.returncode > 0, (name, r.returncode)
        assert "triangulation" in r.stderr or "Camera" in r.stderr, (name, r.stderr[-300:])
        t = tables(db)
        assert not t["matches"] and t["tracks"] is None and t["points3D"] is None, name     # nothing was matched
