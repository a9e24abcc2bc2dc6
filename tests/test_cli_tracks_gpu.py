"""`ComputeMatches <yaml>` with SIFTmatch.tracks : 1 on a synth.south_building_database: the `tracks` table equals the numpy reference
(tests/tracks_ref.py) fed with the `matches` table the run wrote -- under device verification (the device folds its chunks), host
verification and the emission options (the stored rows go through msfm_tracks_add), on a partly filled database (the rows that were
there are read back and added), with one ordinal named twice in MSFM_DEVICES (two contexts, forests joined by export / import) and
with MSFM_EMIT_ORDER=pair_id; without the key there is no `tracks` table; `matches` and stdout are byte for byte what they are without
the key.  Exact equality everywhere."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tracks_ref
from monocularsfm_amd import database, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
EXE = os.path.join(HOST, "ComputeMatches")
YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : 1
{extra}"""
N_IMG = 24
MIN_MATCHES = 10       # the key's default: MapBuilder::Parameters::min_num_matches


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tracks") / "base.db")
    descs, _ = synth.south_building_database(path, N_IMG, 500, seed=91)
    return path, [len(d) for d in descs]


def copy_db(src, dst):
    shutil.copy(src, dst)
    for ext in ("-wal", "-shm"):
        if os.path.exists(src + ext):
            shutil.copy(src + ext, dst + ext)
    return dst


def run(exe, tmp_path, db, tracks, env_extra=None, extra=""):
    cfg = tmp_path / (os.path.basename(db) + ".yaml")
    cfg.write_text(YAML.format(db=db, extra=("SIFTmatch.tracks : 1\n" if tracks else "") + extra))
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def tables(path):
    db = database.Database(path)
    m = db.db.execute("SELECT pair_id, rows, cols, data FROM matches ORDER BY pair_id").fetchall()
    has = db.db.execute("SELECT count(*) FROM sqlite_master WHERE name = 'tracks'").fetchone()[0]
    t = db.db.execute("SELECT track_id, length, consistent, elements FROM tracks ORDER BY track_id").fetchall() if has else None
    ids = [r[0] for r in db.db.execute("SELECT image_id FROM images ORDER BY image_id")]
    db.Close()
    return m, t, ids


def reference(matches, ids, rows, **kw):
    """tracks_ref over the stored rows: pair_id = 10000 * smaller id + larger id, column 0 = the smaller id's keypoint index."""
    pairs = np.asarray([(pid // 10000, pid % 10000) for pid, _, _, _ in matches], np.int32).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum([r for _, r, _, _ in matches])]).astype(np.int64)
    qt = np.concatenate([np.frombuffer(d or b"", "<i4").reshape(-1, 2) for _, _, _, d in matches] + [np.zeros((0, 2), np.int32)])
    return tracks_ref.build(ids, rows, [(pairs, offsets, qt)], kw.pop("min_pair_matches", MIN_MATCHES), **kw)


def check_table(tracks, want):
    assert tracks is not None and len(tracks) == want["stats"]["tracks_kept"]
    o = want["offsets"]
    for t, (track_id, length, consistent, elements) in enumerate(tracks):
        assert track_id == t and length == o[t + 1] - o[t] and consistent == int(want["consistent"][t])
        el = np.frombuffer(elements, "<i4").reshape(-1, 2)
        assert np.array_equal(el[:, 0], want["image_ids"][o[t]:o[t + 1]]) and np.array_equal(el[:, 1], want["point_idx"][o[t]:o[t + 1]])


def strip(s):
    return re.sub(r"\t .*seconds.*\n|.*minutes.*\n|.*\[msfm.*\n|Elapsed.*\n", "", s)   # (the timing lines)


@pytest.fixture(scope="module")
def plain(exe, base, tmp_path_factory):
    """The run without the key: its stdout and its matches table."""
    d = tmp_path_factory.mktemp("plain")
    db = copy_db(base[0], str(d / "off.db"))
    r = run(exe, d, db, False)
    m, t, ids = tables(db)
    assert t is None and len(m) > 100            # without the key there is no tracks table
    return r.stdout, m, ids, db


@pytest.mark.parametrize("env", [{}, {"MSFM_DEVICES": "0,0", "MSFM_SUPER_BATCH_PAIRS": "16"}, {"MSFM_EMIT_ORDER": "pair_id"},
                                 {"MSFM_MAX_PAIRS_PER_BATCH": "9"}],
                         ids=["one-context", "ordinal-twice", "emit-pair-id", "many-sub-batches"])
def test_device_verification(exe, base, plain, tmp_path, env):
    stdout_off, m_off, ids, _ = plain
    db = copy_db(base[0], str(tmp_path / "on.db"))
    r = run(exe, tmp_path, db, True, dict(env, MSFM_CLI_TIMING="1"))
    m, t, _ = tables(db)
    assert m == m_off and strip(r.stdout) == strip(stdout_off)
    assert len(re.findall(r"^\[msfm tracks\] ", r.stderr, re.M)) == 1
    want = reference(m, ids, base[1])
    check_table(t, want)
    assert want["stats"]["tracks_kept"] > 50 and want["stats"]["longest_track"] >= 3 and want["stats"]["pairs_below_min"] > 0


def test_filter_keys(exe, base, plain, tmp_path):
    db = copy_db(base[0], str(tmp_path / "f.db"))
    run(exe, tmp_path, db, True, extra="SIFTmatch.tracks_min_num_matches : 25\nSIFTmatch.tracks_min_length : 3\nSIFTmatch.tracks_max_length : 8\n"
                                       "SIFTmatch.tracks_keep_inconsistent : 1\n")
    m, t, ids = tables(db)
    assert m == plain[1]
    want = reference(m, ids, base[1], min_pair_matches=25, min_length=3, max_length=8, keep_inconsistent=True)
    check_table(t, want)
    assert 0 < want["stats"]["tracks_kept"] < reference(m, ids, base[1])["stats"]["tracks_kept"]


@pytest.mark.parametrize("env", [{"MSFM_GEOMETRIC_VERIFICATION": "host"}, {"MSFM_GEOMETRIC_VERIFICATION": "host", "MSFM_DEVICES": "0,0"},
                                 {"MSFM_SCENEGRAPH_MIN_MATCHES": "30"}], ids=["host-ransac", "host-ransac-two-contexts", "rows-0-below-30"])
def test_stored_rows_that_are_not_the_devices_lists(exe, base, tmp_path, env):
    off, on = copy_db(base[0], str(tmp_path / "off.db")), copy_db(base[0], str(tmp_path / "on.db"))
    r_off = run(exe, tmp_path, off, False, env)
    r_on = run(exe, tmp_path, on, True, env)
    m_off, t_off, ids = tables(off)
    m, t, _ = tables(on)
    assert t_off is None and m == m_off and strip(r_on.stdout) == strip(r_off.stdout)
    want = reference(m, ids, base[1])
    check_table(t, want)
    assert want["stats"]["tracks_kept"] > 20
    if "MSFM_SCENEGRAPH_MIN_MATCHES" in env:
        assert any(r[1] == 0 for r in m)          # rows stored with rows = 0 contribute nothing: the table and the tracks agree


def test_partly_filled_database(exe, base, plain, tmp_path):
    """A resumed run: half of the rows are in the table already (read back, column swap undone, msfm_tracks_add), the other half is
    computed; and a run that computes nothing rebuilds the table from the rows alone."""
    _, m_full, ids, full_db = plain
    db = copy_db(full_db, str(tmp_path / "half.db"))
    con = database.Database(db)
    con.db.execute("DELETE FROM matches WHERE pair_id % 2 = 0")
    con.db.commit()
    con.Close()
    r = run(exe, tmp_path, db, True)
    m, t, _ = tables(db)
    assert m == m_full and "Existing, Continue!" in r.stdout
    want = reference(m, ids, base[1])
    check_table(t, want)
    r2 = run(exe, tmp_path, db, True, extra="SIFTmatch.tracks_min_length : 3\n")     # everything exists: rebuilt whole, another filter
    m2, t2, _ = tables(db)
    assert m2 == m_full
    check_table(t2, reference(m2, ids, base[1], min_length=3))
    assert len(t2) < len(t)
