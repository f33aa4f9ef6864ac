"""The key-frame graph walks of hs_kf_votes / hs_kf_redundancy (include/hyslam_amd.h) restated from the reference's text, twice:

  votes_literal / redundancy_literal   dicts and lists, statement by statement after CovisNode::UpdateConnections (src/core/CovisibilityGraph.cpp:
                                       42-124), TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:80-123) and
                                       KeyFrameCuller::run (src/slam/mapping/KeyFrameCuller.cpp:21-93)
  votes_fast / redundancy_fast         numpy, for the larger cases

A key frame is its slot: the position in ascending KeyFrame* order, so iterating a std::map<KeyFrame*, ...> is iterating ascending slots (DESIGN.md
D11).  A table is a dict of numpy arrays named as the fields of hs_kf_table.  Integer arithmetic only; the one float product of the culler's verdict
goes through numpy.float32.  tests/test_kfgraph_ref.py pins the two versions against each other and against hand-derived answers."""
import numpy as np


def _observations(T, lm):
    b, e = int(T["lm_obs_offsets"][lm]), int(T["lm_obs_offsets"][lm + 1])
    return [(int(T["lm_obs_kf"][j]), int(T["lm_obs_octave"][j])) for j in range(b, e)]       # std::map<KeyFrame*, size_t>: ascending slots


def votes_literal_one(T, q_lm, self_id, count_bad_kf, th):
    """one query -> (KFcounter as {slot: count}, max_slot, max_count, [(slot, weight)] in mvpOrderedConnectedKeyFrames order)"""
    counter = {}
    for lm in q_lm:                                                   # for(vit = spMP.begin() ...) / for(it = matches.cbegin() ...)
        lm = int(lm)
        if T["lm_bad"][lm]:                                           # if(pMP->isBad()) continue;
            continue
        for slot, _ in _observations(T, lm):
            if self_id != -1 and int(T["kf_id"][slot]) == self_id:    # if(pKF_obs->mnId==pKF_node->mnId) continue;
                continue
            if not count_bad_kf and T["kf_bad"][slot]:                # if(pKF_obs->isBad()) continue;   (UpdateLocalKeyFrames counts them)
                continue
            counter[slot] = counter.get(slot, 0) + 1                  # KFcounter[mit->first]++;
    if not counter:                                                   # if(KFcounter.empty()) return;
        return counter, -1, 0, []
    nmax, kfmax, pairs = 0, None, []
    for slot in sorted(counter):                                      # for(mit = KFcounter.begin() ...)
        c = counter[slot]
        if count_bad_kf and T["kf_bad"][slot]:                        # if(pKF->isBad()) continue;       (TrackLocalMap.cpp:113)
            continue
        if c > nmax:
            nmax, kfmax = c, slot
        if c >= th:
            pairs.append((c, slot))                                   # vPairs.push_back(make_pair(mit->second, mit->first));
    if not pairs and kfmax is not None:                               # if(vPairs.empty()) vPairs.push_back(make_pair(nmax, pKFmax));
        pairs.append((nmax, kfmax))
    pairs.sort()                                                      # sort(vPairs.begin(), vPairs.end());
    ordered = []
    for c, slot in pairs:                                             # lKFs.push_front(...); lWs.push_front(...);
        ordered.insert(0, (slot, c))
    return counter, (-1 if kfmax is None else kfmax), nmax, ordered


def _pack_votes(n_kf, cap, rows):
    Q = len(rows)
    out = dict(weights=np.zeros((Q, n_kf), np.int32), max_slot=np.zeros(Q, np.int32), max_count=np.zeros(Q, np.int32),
               ordered_slot=np.full((Q, cap), -1, np.int32), ordered_weight=np.zeros((Q, cap), np.int32), n_ordered=np.zeros(Q, np.int32),
               ordered=[])
    for q, (w, ms, mc, ordered) in enumerate(rows):
        out["weights"][q] = w
        out["max_slot"][q], out["max_count"][q], out["n_ordered"][q] = ms, mc, len(ordered)
        for i, (slot, c) in enumerate(ordered[:cap]):
            out["ordered_slot"][q, i], out["ordered_weight"][q, i] = slot, c
        out["ordered"].append(ordered)                                # the untruncated lists = the symmetric updates (:96,103)
    return out


def votes_literal(T, q_offsets, q_lm, self_id=None, count_bad_kf=False, th=15, cap=10):
    n_kf, rows = len(T["kf_id"]), []
    for q in range(len(q_offsets) - 1):
        counter, ms, mc, ordered = votes_literal_one(T, q_lm[int(q_offsets[q]):int(q_offsets[q + 1])], -1 if self_id is None else int(self_id[q]),
                                                     count_bad_kf, th)
        w = np.zeros(n_kf, np.int32)
        for slot, c in counter.items():
            w[slot] = c
        rows.append((w, ms, mc, ordered))
    return _pack_votes(n_kf, cap, rows)


def _expand(T, lms):
    """the observations of the landmarks `lms`: (index into lms of every observation, index into the table's observation arrays)"""
    off = T["lm_obs_offsets"]
    start, n = off[lms], off[lms + 1] - off[lms]
    owner = np.repeat(np.arange(len(lms)), n)
    first = np.cumsum(n) - n
    return owner, (np.arange(int(n.sum())) - first[owner] + start[owner]).astype(np.int64)


def votes_fast(T, q_offsets, q_lm, self_id=None, count_bad_kf=False, th=15, cap=10):
    n_kf, rows = len(T["kf_id"]), []
    q_lm = np.asarray(q_lm, np.int64)
    bad_kf = np.asarray(T["kf_bad"]) != 0
    for q in range(len(q_offsets) - 1):
        lms = q_lm[int(q_offsets[q]):int(q_offsets[q + 1])]
        lms = lms[np.asarray(T["lm_bad"])[lms] == 0]
        _, idx = _expand(T, lms)
        slots = np.asarray(T["lm_obs_kf"])[idx]
        keep = np.ones(len(slots), bool)
        if self_id is not None and int(self_id[q]) != -1:
            keep &= np.asarray(T["kf_id"])[slots] != int(self_id[q])
        if not count_bad_kf:
            keep &= ~bad_kf[slots]
        w = np.bincount(slots[keep], minlength=n_kf).astype(np.int32)
        elig = (w > 0) & ~(bad_kf if count_bad_kf else np.zeros(n_kf, bool))
        if elig.any():
            mc = int(w[elig].max())
            ms = int(np.nonzero(elig & (w == mc))[0][0])
            idx = np.nonzero(elig & (w >= th))[0]
            if len(idx) == 0:
                idx = np.array([ms])
            order = np.lexsort((-idx, -w[idx].astype(np.int64)))
            ordered = [(int(idx[i]), int(w[idx[i]])) for i in order]
        else:
            ms, mc, ordered = -1, 0, []
        rows.append((w, ms, mc, ordered))
    return _pack_votes(n_kf, cap, rows)


def redundancy_literal(T, cand_slot, cand_th_depth, cand_offsets, item_lm, item_octave, item_depth, is_mono=False, th_obs=3, frac_redundant=0.9):
    C = len(cand_slot)
    out = dict(n_mps=np.zeros(C, np.int32), n_redundant=np.zeros(C, np.int32), cull=np.zeros(C, np.uint8))
    for c in range(C):
        me = int(cand_slot[c])
        n_redundant, n_mps = 0, 0                                     # int nRedundantObservations=0; int nMPs=0;
        for k in range(int(cand_offsets[c]), int(cand_offsets[c + 1])):
            lm = int(item_lm[k])
            if T["lm_bad"][lm]:                                       # if(!pMP->isBad())
                continue
            if not is_mono:
                depth = np.float32(item_depth[k])
                if depth > np.float32(cand_th_depth[c]) or depth < 0:  # if(depth_pt > pKFi->mThDepth || depth_pt < 0) continue;
                    continue
            n_mps += 1
            if int(T["lm_nobs"][lm]) > th_obs:                        # if(pMP->Observations()>thObs)
                level = int(item_octave[k])
                n_obs = 0
                for slot, octave in _observations(T, lm):
                    if slot == me:                                    # if(pKFi2==pKFi) continue;
                        continue
                    if octave <= level + 1:                           # if(scaleLeveli<=scaleLevel+1)
                        n_obs += 1
                        if n_obs >= th_obs:
                            break
                if n_obs >= th_obs:
                    n_redundant += 1
        out["n_mps"][c], out["n_redundant"][c] = n_mps, n_redundant
        out["cull"][c] = np.float32(n_redundant) > np.float32(frac_redundant) * np.float32(n_mps)   # int > float * int (:86)
    return out


def redundancy_fast(T, cand_slot, cand_th_depth, cand_offsets, item_lm, item_octave, item_depth, is_mono=False, th_obs=3, frac_redundant=0.9):
    C = len(cand_slot)
    out = dict(n_mps=np.zeros(C, np.int32), n_redundant=np.zeros(C, np.int32), cull=np.zeros(C, np.uint8))
    item_lm, item_octave = np.asarray(item_lm, np.int64), np.asarray(item_octave, np.int64)
    for c in range(C):
        b, e = int(cand_offsets[c]), int(cand_offsets[c + 1])
        lm, level = item_lm[b:e], item_octave[b:e]
        keep = np.asarray(T["lm_bad"])[lm] == 0
        if not is_mono:
            d = np.asarray(item_depth, np.float32)[b:e]
            keep &= ~((d > np.float32(cand_th_depth[c])) | (d < 0))
        lm, level = lm[keep], level[keep]
        n_mps = len(lm)
        use = np.asarray(T["lm_nobs"])[lm] > th_obs
        lm, level = lm[use], level[use]
        owner, idx = _expand(T, lm)
        ok = (np.asarray(T["lm_obs_kf"])[idx] != int(cand_slot[c])) & (np.asarray(T["lm_obs_octave"])[idx] <= level[owner] + 1)
        n_red = int((np.bincount(owner[ok], minlength=len(lm)) >= th_obs).sum())
        out["n_mps"][c], out["n_redundant"][c] = n_mps, n_red
        out["cull"][c] = np.float32(n_red) > np.float32(frac_redundant) * np.float32(n_mps)
    return out


VOTE_KEYS = ("weights", "max_slot", "max_count", "ordered_slot", "ordered_weight", "n_ordered")
RED_KEYS = ("n_mps", "n_redundant", "cull")


def same(got, want, keys):
    """every output identical; returns the first key that differs (None: all equal)"""
    for k in keys:
        if got[k] is None:
            continue
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            return k
    return None
