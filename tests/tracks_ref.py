"""Independent reference of the feature tracks (include/msfm_match.h "feature tracks"), written from the definitions in plain numpy:
components by min-label propagation with pointer jumping (no union-find), everything else by sorting.  Test infrastructure only.

    nodes       images ranked by ascending id; node = base[rank] + keypoint index, base the exclusive prefix sum of the rows
    per pair    an undeclared image -> skipped; id1 == id2 -> all matches ignored; fewer than min_pair_matches matches -> nothing;
                else folded, a match with an index outside [0, rows) ignored, every other one an edge
    track       a connected component of >= 2 nodes; consistent iff no two nodes of one image
    kept        max(2, min_length) <= length, length <= max_length (0: no bound), consistent unless keep_inconsistent
    order       kept tracks by ascending smallest node, elements by ascending node
"""
import numpy as np

COUNT_KEYS = ("nodes", "edges", "pairs", "pairs_skipped", "pairs_below_min", "matches_ignored", "tracks_total", "tracks_inconsistent",
              "tracks_over_max_length", "tracks_kept", "observations_kept", "longest_track")


def numbering(ids, rows):
    ids = np.asarray(ids, np.int64).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    order = np.argsort(ids, kind="stable")
    sid, srows = ids[order], rows[order]
    assert len(np.unique(sid)) == len(sid), "ids must be distinct"
    base = np.concatenate([[0], np.cumsum(srows)]).astype(np.int64)
    return sid, srows, base


def edges_of(sid, srows, base, lists, min_pair_matches, counts):
    """The node pairs (a, b) of every edge of `lists` = iterable of (pairs P x 2, offsets P + 1, qt M x 2); counts is updated."""
    ea, eb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for pairs, offsets, qt in lists:
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        offsets = np.asarray(offsets, np.int64).reshape(-1)
        qt = np.asarray(qt, np.int64).reshape(-1, 2)
        P = len(pairs)
        if P == 0:
            continue
        length = np.diff(offsets)
        rank = np.searchsorted(sid, pairs)
        rank_c = np.minimum(rank, max(len(sid) - 1, 0))
        declared = (sid[rank_c] == pairs) if len(sid) else np.zeros_like(pairs, bool)
        skipped = ~(declared[:, 0] & declared[:, 1])
        self_pair = ~skipped & (pairs[:, 0] == pairs[:, 1])
        below = ~skipped & ~self_pair & (length < min_pair_matches)
        fold = ~skipped & ~self_pair & ~below
        counts["pairs_skipped"] += int(skipped.sum())
        counts["matches_ignored"] += int(length[self_pair].sum())
        counts["pairs_below_min"] += int(below.sum())
        counts["pairs"] += int(fold.sum())
        pair_of = np.repeat(np.arange(P), length)
        m = qt[offsets[0]:offsets[-1]]
        keep = fold[pair_of]
        pair_of, m = pair_of[keep], m[keep]
        r1, r2 = rank_c[pair_of, 0], rank_c[pair_of, 1]
        ok = (m[:, 0] >= 0) & (m[:, 0] < srows[r1]) & (m[:, 1] >= 0) & (m[:, 1] < srows[r2])
        counts["matches_ignored"] += int((~ok).sum())
        counts["edges"] += int(ok.sum())
        ea.append(base[r1[ok]] + m[ok, 0])
        eb.append(base[r2[ok]] + m[ok, 1])
    return np.concatenate(ea), np.concatenate(eb)


def components(n, a, b):
    """label[v] = the smallest node of v's component."""
    label = np.arange(n, dtype=np.int64)
    while len(a):
        la, lb = label[a], label[b]
        lo = np.minimum(la, lb)
        if np.array_equal(la, lb):
            break
        np.minimum.at(label, la, lo)     # the labels' own labels first (hooking), then the endpoints
        np.minimum.at(label, lb, lo)
        np.minimum.at(label, a, lo)
        np.minimum.at(label, b, lo)
        while True:                      # pointer jumping
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
    return label


def build(ids, rows, lists, min_pair_matches=0, min_length=2, max_length=0, keep_inconsistent=False, forests=()):
    """-> dict(stats, offsets, image_ids, point_idx, consistent, track_ids {image id: int32 per keypoint}, label).  forests: arrays of
    one entry per node, each joined with its node (msfm_tracks_import_forest)."""
    sid, srows, base = numbering(ids, rows)
    n = int(base[-1])
    counts = {k: 0 for k in COUNT_KEYS}
    counts["nodes"] = n
    a, b = edges_of(sid, srows, base, lists, min_pair_matches, counts)
    for f in forests:
        f = np.asarray(f, np.int64).reshape(-1)
        assert len(f) == n and (f >= 0).all() and (f < n).all()
        a = np.concatenate([a, np.arange(n, dtype=np.int64)])
        b = np.concatenate([b, f])
    label = components(n, a, b)
    size = np.bincount(label, minlength=max(n, 1))
    nodes = np.nonzero(size[label] >= 2)[0] if n else np.zeros(0, np.int64)
    nodes = nodes[np.lexsort((nodes, label[nodes]))]
    lab = label[nodes]
    img = np.searchsorted(base, nodes, side="right") - 1
    head = np.ones(len(nodes), bool)
    head[1:] = lab[1:] != lab[:-1]
    track = np.cumsum(head) - 1                                  # number among ALL tracks
    n_tracks = int(head.sum())
    clash = np.zeros(len(nodes), bool)
    clash[1:] = (lab[1:] == lab[:-1]) & (img[1:] == img[:-1])
    inconsistent = np.zeros(n_tracks, bool)
    inconsistent[track[clash]] = True
    length = np.bincount(track, minlength=n_tracks)
    over = (length > max_length) if max_length > 0 else np.zeros(n_tracks, bool)
    kept = (length >= max(2, min_length)) & ~over & (~inconsistent | bool(keep_inconsistent))
    counts["tracks_total"] = n_tracks
    counts["tracks_inconsistent"] = int(inconsistent.sum())
    counts["tracks_over_max_length"] = int(over.sum())
    counts["tracks_kept"] = int(kept.sum())
    counts["observations_kept"] = int(length[kept].sum())
    counts["longest_track"] = int(length[kept].max()) if kept.any() else 0
    new_number = np.cumsum(kept) - 1
    el = kept[track] if len(nodes) else np.zeros(0, bool)
    offsets = np.concatenate([[0], np.cumsum(length[kept])]).astype(np.int64)
    image_ids = sid[img[el]].astype(np.int32)
    point_idx = (nodes[el] - base[img[el]]).astype(np.int32)
    track_of = np.full(n, -1, np.int32)
    track_of[nodes[el]] = new_number[track[el]]
    track_ids = {int(sid[p]): track_of[base[p]:base[p + 1]] for p in range(len(sid))}
    return {"stats": counts, "offsets": offsets, "image_ids": image_ids, "point_idx": point_idx,
            "consistent": (~inconsistent[kept]).astype(np.uint8), "track_ids": track_ids, "label": label}
