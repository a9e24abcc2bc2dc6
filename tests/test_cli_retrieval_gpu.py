"""`ComputeMatches` in matching mode 2 (vocabulary retrieval) on a planted co-visibility database: rows for exactly the retrieved pairs,
each row byte-identical to what the matching path writes for that pair, the usual stdout, resume, several contexts, the Python mirror."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from monocularsfm_amd import _lib, database, synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import retrieval_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
EXE = os.path.join(HOST, "ComputeMatches")
K, WORDS = 4, 256

YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : {mt}
SIFTmatch.num_nearest_images : {k}
SIFTmatch.vocab_num_words : {v}
SIFTmatch.vocab_train_iters : 8
"""


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def scene():
    # every prototype once per image that sees it: a row's nearest neighbour in an overlapping image is its own prototype's copy
    images, overlap = ref.covis_scene(16, window=300, stride=40, per_proto=1, fresh=60, jitter=3, seed=9, as_float=True)
    descs = [np.ascontiguousarray(images[i], np.float32) for i in range(len(images))]
    kps = [synth.keypoints(len(d), seed=70 + i) for i, d in enumerate(descs)]
    return descs, kps


def run_cli(exe, cfg, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def rows_of(path):
    d = database.Database(path)
    r = d.db.execute("SELECT pair_id, rows, cols, data FROM matches ORDER BY pair_id").fetchall()
    d.Close()
    return r


def _db(tmp_path, name, scene, mt=2):
    descs, kps = scene
    path = str(tmp_path / (name + ".db"))
    database.write_synthetic_database(path, descs, kps)
    cfg = tmp_path / (name + ".yaml")
    cfg.write_text(YAML.format(db=path, mt=mt, k=K, v=WORDS))
    return path, cfg


def test_mode_2_writes_the_retrieved_pairs(exe, scene, gpu_ctx, tmp_path):
    descs, kps = scene
    path, cfg = _db(tmp_path, "vocab", scene)
    out = run_cli(exe, cfg)
    # the pairs: the library's retrieval on the same images
    gpu_ctx.clear_images()
    for i, d in enumerate(descs):
        gpu_ctx.upload_image(i, d)
        gpu_ctx.upload_keypoints(i, kps[i])
    ids = list(range(len(descs)))
    gpu_ctx.train_vocabulary(ids, num_words=WORDS, train_iters=8)
    pairs, _ = gpu_ctx.retrieve_pairs(ids, K)
    pairs = [tuple(p) for p in pairs.tolist()]
    assert len(descs) - 1 <= len(pairs) < len(descs) * (len(descs) - 1) // 2
    got = rows_of(path)
    assert sorted(r[0] for r in got) == sorted(database.ImagePairToPairId(i, j) for i, j in pairs)
    # every row is the matching path's row for that pair (geometric verification on the device: the CLI's default)
    offs, qt, _ = gpu_ctx.match_pairs_verified(np.asarray(pairs, np.int32))
    db = database.Database(path)
    for p, (i, j) in enumerate(pairs):
        assert np.array_equal(db.ReadMatches(i, j), qt[offs[p]:offs[p + 1]]), (i, j)
    db.Close()
    # stdout: the summary line, the usual per-pair lines in brute mode's order
    assert re.search(r"Vocabulary retrieval: 16 images, %d words, %d nearest, %d pairs, [0-9.]+ s\n" % (WORDS, K, len(pairs)), out)
    seen = [tuple(map(int, m)) for m in re.findall(r"Compute Matches (\d+) - (\d+) \.\.\. \n", out)]
    assert seen == pairs
    assert re.search(r"\t matches num : \d+\n\t Elapsed time: \d+\.\d{5} \[seconds\]\n", out)
    # a re-run skips every existing row
    out2 = run_cli(exe, cfg)
    assert out2.count("Existing, Continue!") == len(pairs) and " ... " not in out2
    assert rows_of(path) == got


def test_mode_2_rows_equal_brute_mode_rows(exe, scene, tmp_path):
    # (verification off: the distance-filtered lists themselves; brute mode's pre-emptive filter leaves some pairs without a row)
    a, ca = _db(tmp_path, "vocab", scene, mt=2)
    b, cb = _db(tmp_path, "brute", scene, mt=1)
    run_cli(exe, ca, {"MSFM_GEOMETRIC_VERIFICATION": "0"})
    run_cli(exe, cb, {"MSFM_GEOMETRIC_VERIFICATION": "0"})
    brute = {r[0]: r for r in rows_of(b)}
    vocab = rows_of(a)
    shared = [r for r in vocab if r[0] in brute]
    assert len(shared) >= 5 and any(r[1] > 0 for r in shared)
    for r in shared:
        assert r == brute[r[0]]


def test_mode_2_several_contexts_and_python_mirror(exe, scene, gpu_ctx, tmp_path):
    from monocularsfm_amd.matcher import VocabularyTreeFeatureMatcher
    a, ca = _db(tmp_path, "one", scene)
    b, cb = _db(tmp_path, "two", scene)
    c = str(tmp_path / "py.db")
    shutil.copy(a, c)
    out_a = run_cli(exe, ca)
    out_b = run_cli(exe, cb, {"MSFM_DEVICES": "0,0"})
    strip = lambda s: re.sub(r"(Elapsed time: |pairs, )[0-9.]+", r"\1X", s)
    assert strip(out_a) == strip(out_b)
    assert rows_of(a) == rows_of(b) and len(rows_of(a)) > 10
    gpu_ctx.clear_images()
    VocabularyTreeFeatureMatcher(c, num_nearest_images=K, vocab_num_words=WORDS, vocab_train_iters=8, ctx=gpu_ctx, verbose=False,
                                 geometric_verification="device").RunMatching()
    assert rows_of(c) == rows_of(a)


def test_other_match_types_still_abort(exe, scene, tmp_path):
    path, cfg = _db(tmp_path, "bad", scene, mt=3)
    r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "match_type" in r.stderr
