"""Independent numpy restatement of the vocabulary-grouped matchers and what feeds them (test infrastructure), in the manner of tests/pyref.py.

Written from the reference's text — FeatureMatcher.cc:216-402 (SearchByBoW, _SearchByBoW_, SearchByBoW2, SearchForTriangulation), :938-1120 (the legacy
SearchByBoW(pKF1, pKF2, ...) and ComputeThreeMaxima), MatchCriteria.cpp:551-767 (index criteria, BestMatchBoWCriterion, EpipolarConsistencyBoWCriterion,
RotationConsistency), FeatureExtractorSettings.cpp:5-8 (determineSigma2), Frame.cc:472-479 — and, for DBoW2 (not part of the reference tree), from the
published algorithm as include/hyslam_amd.h cites it.  It shares no code with oracle/ or the kernels: each side-1 feature is answered from a whole
Hamming matrix of its node instead of a running best / second-best scan.

Arithmetic: every product and sum the reference does in `float` is one float32 numpy operation (the epipolar line, num*num/den, rot, rot*factor,
ratio*bestDist2, 0.1f*max1); `3.84*sigma2` is a double product of the float sigma2; std::round is half away from zero; comparisons strict as written.

Input domain (outside it the reference has undefined behaviour or an assert): key-point angles finite and in [0, 360); node ids ascending and unique
per feature vector; a feature index appears at most once in a feature vector (in one node, once); indices inside [0, n)."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
HISTO_LENGTH = 30
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
_FAR = 1 << 20                                            # stands for "not a candidate" in a distance matrix


def hamming_matrix(A, B):
    """(len(A), len(B)) Hamming distances of 32-byte descriptors"""
    A = np.asarray(A, np.uint8).reshape(-1, 32); B = np.asarray(B, np.uint8).reshape(-1, 32)
    out = np.zeros((len(A), len(B)), np.int32)
    step = max(1, (1 << 22) // max(len(B) * 32, 1))
    for s in range(0, len(A), step):
        out[s:s + step] = _POP[A[s:s + step, None, :] ^ B[None, :, :]].sum(2)
    return out


def _round_away(a):
    a = np.asarray(a, np.float64)
    return np.sign(a) * np.floor(np.abs(a) + 0.5)


def three_maxima(counts):
    """ComputeThreeMaxima on the bin sizes -> (ind1, ind2, ind3), -1 = none.  Strict `>` while scanning, so the first of equal bins ranks higher;
    a runner-up below 0.1f * max1 (float product, the int compared as float) is dropped together with what ranks below it."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    lim = f32(0.1) * f32(max1)
    if f32(max2) < lim:
        ind2 = ind3 = -1
    elif f32(max3) < lim:
        ind3 = -1
    return ind1, ind2, ind3


def rotation_bins(angle_from, angle_to):
    """bin of rot = angle_to - angle_from (float), +360 when negative, bin = round(rot * (1.0f / 30)), 30 -> 0.  -> (bins int64, rot * factor float32)"""
    with np.errstate(all="ignore"):
        rot = (np.asarray(angle_to, f32) - np.asarray(angle_from, f32)).astype(f32)
        rot = np.where(rot < 0.0, (rot + f32(360.0)).astype(f32), rot).astype(f32)
        scaled = (rot * (f32(1.0) / f32(HISTO_LENGTH))).astype(f32)
    b = _round_away(scaled).astype(np.int64)
    b[b == HISTO_LENGTH] = 0
    assert ((b >= 0) & (b < HISTO_LENGTH)).all(), "angles outside the reference's domain"
    return b, scaled


def rotation_consistency(angle_from, angle_to):
    """RotationConsistency over a match list: keep[i] = the pair's bin is one of the (up to) three maxima.  rot = angle_to - angle_from."""
    b, _ = rotation_bins(angle_from, angle_to)
    keep_bins = [i for i in three_maxima(np.bincount(b, minlength=HISTO_LENGTH)) if i >= 0]
    return np.isin(b, keep_bins)


def _shared_nodes(ids1, ids2, stats=None):
    """the merge walk of two DBoW2::FeatureVector maps: equal keys are visited, a smaller key jumps by lower_bound to the other side's key"""
    out = []
    a = b = 0
    n1, n2 = len(ids1), len(ids2)
    while a < n1 and b < n2:
        if ids1[a] == ids2[b]:
            out.append((a, b)); a += 1; b += 1
        elif ids1[a] < ids2[b]:
            j = int(np.searchsorted(ids1, ids2[b], side="left"))
            if stats is not None:
                stats["skipped1"] = stats.get("skipped1", 0) + (j - a)
            a = j
        else:
            j = int(np.searchsorted(ids2, ids1[a], side="left"))
            if stats is not None:
                stats["skipped2"] = stats.get("skipped2", 0) + (j - b)
            b = j
    return out


def _epipolar_ok(k1, k2, F12, size_ref, sigma_ref, stats=None):
    """EpipolarConsistencyBoWCriterion for every pair: (len(k1), len(k2)) bool.  l = x1' F12, dsqr = num*num/den < 3.84*sigma2(kp2.size)"""
    F = np.asarray(F12, f32).reshape(3, 3)
    with np.errstate(all="ignore"):
        x1, y1 = k1["x"].astype(f32), k1["y"].astype(f32)
        a = (((x1 * F[0, 0]).astype(f32) + (y1 * F[1, 0]).astype(f32)).astype(f32) + F[2, 0]).astype(f32)
        b = (((x1 * F[0, 1]).astype(f32) + (y1 * F[1, 1]).astype(f32)).astype(f32) + F[2, 1]).astype(f32)
        c = (((x1 * F[0, 2]).astype(f32) + (y1 * F[1, 2]).astype(f32)).astype(f32) + F[2, 2]).astype(f32)
        x2, y2 = k2["x"].astype(f32)[None, :], k2["y"].astype(f32)[None, :]
        num = (((a[:, None] * x2).astype(f32) + (b[:, None] * y2).astype(f32)).astype(f32) + c[:, None]).astype(f32)
        den = ((a * a).astype(f32) + (b * b).astype(f32)).astype(f32)[:, None]
        dsqr = ((num * num).astype(f32) / den).astype(f32)
        sf = (k2["size"].astype(f32) / f32(size_ref)).astype(f32)
        sigma2 = (f32(sigma_ref) * (sf * sf).astype(f32)).astype(f32)
        bound = 3.84 * sigma2.astype(np.float64)[None, :]
        ok = (den != 0) & (dsqr.astype(np.float64) < bound)
    if stats is not None:
        stats["den0"] = stats.get("den0", 0) + int((den == 0).sum()) * (k2.shape[0] > 0)
        stats["on_bound"] = stats.get("on_bound", 0) + int(((den != 0) & (dsqr.astype(np.float64) == bound)).sum())
        stats["nonfinite"] = stats.get("nonfinite", 0) + int((~np.isfinite(dsqr) & (den != 0)).sum())
    return ok


def _best_two(D, allowed):
    """per row of a distance matrix: position of the first minimum among allowed columns (-1: none), bestDist1, bestDist2 as float32 (FLT_MAX
    when absent): the second smallest of the multiset, equal to the best on a tie"""
    n = D.shape[0]
    if D.shape[1] == 0:
        return np.full(n, -1, np.int64), np.full(n, FLT_MAX, f32), np.full(n, FLT_MAX, f32)
    M = np.where(allowed, D, _FAR)
    pos = M.argmin(1)                                                        # first occurrence = first in list order
    cnt = allowed.sum(1)
    b1 = M[np.arange(n), pos]
    if D.shape[1] > 1:
        b2 = np.partition(M, 1, axis=1)[:, 1]
    else:
        b2 = np.full(n, _FAR)
    best1 = np.where(cnt >= 1, b1, 0).astype(f32); best1[cnt < 1] = FLT_MAX
    best2 = np.where(cnt >= 2, b2, 0).astype(f32); best2[cnt < 2] = FLT_MAX
    return np.where(cnt >= 1, pos, -1), best1, best2


def _accept(best1, best2, thr, ratio):
    with np.errstate(all="ignore"):
        return (best1 < f32(thr)) & (best1 < (f32(ratio) * best2).astype(f32))


def search_by_bow(k1, d1, fv1, k2, d2, fv2, keep1, score_threshold, ratio, check_rotation, keep2=None, F12=None, size_ref=31.0, sigma_ref=1.0, stats=None):
    """SearchByBoW (keep1 only), SearchByBoW2 / _SearchByBoW_ (keep1, keep2) and the SearchForTriangulation core (F12 given): for every node both
    feature vectors hold, each side-1 index that passes the index criteria takes the first minimum over the side-2 indices that pass theirs and the
    epipolar criterion, accepted when d < score_threshold and d < ratio * d2; then RotationConsistencyBoW (rot = angle2 - angle1).
    fv = (node_id, node_ptr, idx).  -> (match12 int32 [n1], number of matches).  `stats` (a dict) collects what the generators' self-checks ask for."""
    ids1, ptr1, idx1 = (np.asarray(x, np.int64) for x in fv1)
    ids2, ptr2, idx2 = (np.asarray(x, np.int64) for x in fv2)
    d1 = np.asarray(d1, np.uint8).reshape(-1, 32); d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
    match12 = np.full(len(k1), -1, np.int32)
    for a, b in _shared_nodes(ids1, ids2, stats):
        l1 = idx1[ptr1[a]:ptr1[a + 1]]
        l2 = idx2[ptr2[b]:ptr2[b + 1]]
        if keep1 is not None:
            l1 = l1[np.asarray(keep1)[l1] != 0]
        if keep2 is not None:
            l2 = l2[np.asarray(keep2)[l2] != 0]
        if stats is not None:
            stats.setdefault("sizes1", set()).add(len(l1)); stats.setdefault("sizes2", set()).add(len(l2))
        if len(l1) == 0:
            continue
        D = hamming_matrix(d1[l1], d2[l2])
        allowed = np.ones(D.shape, bool) if F12 is None else _epipolar_ok(k1[l1], k2[l2], F12, size_ref, sigma_ref, stats)
        pos, best1, best2 = _best_two(D, allowed)
        ok = _accept(best1, best2, score_threshold, ratio) & (pos >= 0)
        new = ok & (match12[l1] < 0)                                         # std::map::insert keeps an earlier entry
        match12[l1[new]] = l2[pos[new]]
        if stats is not None:
            cnt = allowed.sum(1)
            stats["ties"] = stats.get("ties", 0) + int(((cnt >= 2) & (best1 == best2)).sum())
            stats["single"] = stats.get("single", 0) + int((cnt == 1).sum())
            stats["at_threshold"] = stats.get("at_threshold", 0) + int(((cnt >= 1) & (best1 == f32(score_threshold))).sum())
            with np.errstate(all="ignore"):
                stats["ratio_edge"] = stats.get("ratio_edge", 0) + int(((cnt >= 2) & (best1 == (f32(ratio) * best2).astype(f32))).sum())
            stats["considered"] = stats.get("considered", 0) + len(l1)
    if check_rotation:
        m = np.nonzero(match12 >= 0)[0]
        if stats is not None and len(m):
            bins, scaled = rotation_bins(k1["angle"][m], k2["angle"][match12[m]])
            _rotation_stats(stats, bins, scaled)
        keep = rotation_consistency(k1["angle"][m], k2["angle"][match12[m]])
        match12[m[~keep]] = -1
    if stats is not None:                                                        # the final outcome per side-1 feature that was looked at
        stats["accepted"] = int((match12 >= 0).sum()); stats["rejected"] = stats.get("considered", 0) - stats["accepted"]
    return match12, int((match12 >= 0).sum())


def _rotation_stats(stats, bins, scaled):
    with np.errstate(all="ignore"):
        frac = scaled.astype(np.float64) - np.floor(scaled.astype(np.float64))
    stats["half_bin"] = stats.get("half_bin", 0) + int((frac == 0.5).sum())
    stats["rot360"] = stats.get("rot360", 0) + int((scaled == f32(f32(360.0) * (f32(1.0) / f32(30)))).sum())
    c = sorted(np.bincount(bins, minlength=HISTO_LENGTH).tolist(), reverse=True)
    lim = f32(0.1) * f32(c[0])
    stats["ten_percent_edge"] = stats.get("ten_percent_edge", 0) + int(any(f32(v) == lim or f32(v + 1) == lim for v in c[1:3] if c[0] >= 10))
    counts = np.bincount(bins, minlength=HISTO_LENGTH)
    kept = [i for i in three_maxima(counts) if i >= 0]
    stats["bins_removed"] = stats.get("bins_removed", 0) + int(sum(1 for i, v in enumerate(counts) if v > 0 and i not in kept))


def search_by_bow_legacy(k1, d1, fv1, k2, d2, fv2, keep1, keep2, th_low, nnratio, check_orientation, stats=None):
    """the legacy SearchByBoW(pKF1, pKF2, vpMatches12): the side-1 features of a shared node in list order; a side-2 feature an earlier one matched
    (vbMatched2) is no candidate any more; d < th_low and d < nnratio * d2; histogram on rot = angle1 - angle2, minority bins removed (the side-2
    features they took stay taken).  -> (match12 int32 [n1], nmatches)"""
    ids1, ptr1, idx1 = (np.asarray(x, np.int64) for x in fv1)
    ids2, ptr2, idx2 = (np.asarray(x, np.int64) for x in fv2)
    d1 = np.asarray(d1, np.uint8).reshape(-1, 32); d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
    match12 = np.full(len(k1), -1, np.int32)
    taken = np.zeros(max(len(k2), 1), bool)
    for a, b in _shared_nodes(ids1, ids2):
        l1 = idx1[ptr1[a]:ptr1[a + 1]]
        l2 = idx2[ptr2[b]:ptr2[b + 1]]
        if keep1 is not None:
            l1 = l1[np.asarray(keep1)[l1] != 0]
        if keep2 is not None:
            l2 = l2[np.asarray(keep2)[l2] != 0]
        if len(l1) == 0 or len(l2) == 0:
            continue
        D = hamming_matrix(d1[l1], d2[l2])
        for r, i1 in enumerate(l1):
            free = ~taken[l2]
            pos, best1, best2 = _best_two(D[r:r + 1], free[None, :])
            if stats is not None and free.any() and not free.all():
                stats["competition"] = stats.get("competition", 0) + int(taken[l2[int(D[r].argmin())]])
            if pos[0] >= 0 and _accept(best1, best2, th_low, nnratio)[0]:
                match12[i1] = l2[pos[0]]
                taken[l2[pos[0]]] = True
        if stats is not None:
            stats["considered"] = stats.get("considered", 0) + len(l1)
    if check_orientation:
        m = np.nonzero(match12 >= 0)[0]
        keep = rotation_consistency(k2["angle"][match12[m]], k1["angle"][m])
        match12[m[~keep]] = -1
    if stats is not None:
        stats["accepted"] = int((match12 >= 0).sum()); stats["rejected"] = stats.get("considered", 0) - stats["accepted"]
    return match12, int((match12 >= 0).sum())


# ---------------------------------------------------------------- DBoW2 transform on the flat tree of the C ABI
def tree_levels(tree):
    """depth of every node of a flat tree (dict with child_begin, child_count): root = 0"""
    cb, cc = np.asarray(tree["child_begin"], np.int64), np.asarray(tree["child_count"], np.int64)
    level = np.zeros(len(cb), np.int64)
    for i in range(len(cb)):
        level[cb[i]:cb[i] + cc[i]] = level[i] + 1
    return level


def bow_transform(tree, desc, levelsup):
    """TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) per descriptor: from the root, move to the child with the smallest
    distance (strict `<` while scanning the children in order: the first minimum wins) until a leaf; word and weight are the leaf's; nid is the
    node passed at level L - levelsup, the root (0) when that level is <= 0, and 0 as well when the leaf lies above it (nid is never assigned).
    With orig_id the reported node is orig_id[nid].  tree: dict(levels, child_begin, child_count, desc, word_id, weight, orig_id | None).
    -> (word int32, weight float32, node int32)"""
    cb, cc = np.asarray(tree["child_begin"], np.int64), np.asarray(tree["child_count"], np.int64)
    nd = np.asarray(tree["desc"], np.uint8).reshape(-1, 32)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    nid_level = int(tree["levels"]) - int(levelsup)
    cur = np.zeros(n, np.int64); nid = np.zeros(n, np.int64)
    level = 0
    active = np.arange(n)
    while len(active):
        level += 1
        for node in np.unique(cur[active]):
            sel = active[cur[active] == node]
            ch = np.arange(cb[node], cb[node] + cc[node])
            cur[sel] = ch[hamming_matrix(desc[sel], nd[ch]).argmin(1)]
        if level == nid_level:
            nid[active] = cur[active]
        active = active[cc[cur[active]] != 0]
    rep = nid if tree.get("orig_id") is None else np.asarray(tree["orig_id"], np.int64)[nid]
    return np.asarray(tree["word_id"], np.int32)[cur].copy(), np.asarray(tree["weight"], f32)[cur].copy(), rep.astype(np.int32)


def feature_vector(word, weight, node):
    """what DBoW2 keeps of a transform: `if (w > 0) fv.addFeature(nid, i)` -> CSR (node ids ascending, node_ptr, feature indices ascending per node)"""
    use = np.nonzero(np.asarray(weight, f32) > 0)[0]
    node = np.asarray(node, np.int64)[use]
    ids = np.unique(node)
    lists = [use[node == i] for i in ids]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    idx = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return ids.astype(np.int32), ptr, idx


def feature_vector_nodes(tree, levelsup):
    """number of distinct keys a feature vector can have: the nodes at level L - levelsup (the root alone when that is <= 0), plus the root when a
    leaf lies above that level"""
    level = tree_levels(tree)
    cc = np.asarray(tree["child_count"], np.int64)
    nid_level = int(tree["levels"]) - int(levelsup)
    if nid_level <= 0:
        return 1
    return int((level == nid_level).sum()) + int(((cc[1:] == 0) & (level[1:] < nid_level)).any())


def hamming_knn2(q, t):
    """brute-force 2-NN: first minimum index, its distance, the second smallest distance of the multiset; -1 where absent"""
    q = np.asarray(q, np.uint8).reshape(-1, 32); t = np.asarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    bi = np.full(nq, -1, np.int32); bd = np.full(nq, -1, np.int32); sd = np.full(nq, -1, np.int32)
    if nq == 0 or nt == 0:
        return bi, bd, sd
    D = hamming_matrix(q, t)
    bi[:] = D.argmin(1)
    bd[:] = D[np.arange(nq), bi]
    if nt > 1:
        sd[:] = np.partition(D, 1, axis=1)[:, 1]
    return bi, bd, sd


def records_bow_match(tree, levelsup, frames, rank, cap, score_threshold, ratio, check_rotation):
    """hs_records_bow_match_device restated: frames = [(kps, desc)] per record (already clamped to the record's count); transform -> feature vector
    -> search_by_bow between record `rank` and every peer.  -> (match12 int32 [world][cap], n_matches int32 [world]); rows beyond the count and the
    `rank` row are -1"""
    world = len(frames)
    fvs = [feature_vector(*bow_transform(tree, d, levelsup)) for k, d in frames]
    out = np.full((world, cap), -1, np.int32)
    nm = np.zeros(world, np.int32)
    k1, d1 = frames[rank]
    for p in range(world):
        if p == rank:
            continue
        m, n = search_by_bow(k1, d1, fvs[rank], frames[p][0], frames[p][1], fvs[p], None, score_threshold, ratio, check_rotation)
        out[p, :len(m)] = m
        nm[p] = n
    return out, nm
