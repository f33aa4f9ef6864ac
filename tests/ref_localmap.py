"""The local map of TrackLocalMap (src/slam/tracking/TrackLocalMap.cpp) between the vote and the projection search — hs_local_keyframes,
hs_local_points, hs_landmark_gather_device (include/hyslam_amd.h) — restated from the reference's text, twice:

  local_keyframes_literal / local_points_literal   a real Python set walked with the iteration rule of std::set (UpdateLocalKeyFrames :106-156), and
                                                   each local key frame's landmark list walked as UpdateLocalPoints does (:166-184), then the filter
                                                   at the head of SearchLocalPoints (:55-67)
  local_keyframes_fast / local_points_fast         arrays; the points straight from the observation table

A key frame is its slot, a landmark its index: the position in ascending address order, so iterating a std::set<KeyFrame*> or a std::set<MapPoint*>
is iterating ascending numbers.  The literal points version reads KeyFrame::GetMapPointMatches(), the table lists the landmarks'
observations: the same relation while associations are symmetric — key_frame_matches() builds the one from the other, and that the
two versions agree pins the decision.  tests/test_localmap_ref.py compares the versions with each other and with the hand-derived answers of
tests/localmap_cases.py."""
import numpy as np


def _exceeds(size, n_max):
    """local_key_frames.size() > params.N_max_local_keyframes: size_t against int, the int converted (a negative one becomes huge)"""
    return size > (n_max if n_max >= 0 else n_max + (1 << 64))


def local_keyframes_literal(weights, kf_bad, neigh, parent, n_max, n_neighbor):
    """-> the set local_key_frames after UpdateLocalKeyFrames, given keyframeCounter = {slot: weights[slot] > 0}"""
    counter = {s: int(w) for s, w in enumerate(weights) if w > 0}                 # std::map<KeyFrame*, int> keyframeCounter
    local = set()                                                                 # local_key_frames.clear()
    if not counter:                                                               # if(keyframeCounter.empty()) return;
        return local
    for s in sorted(counter):                                                     # for(it = keyframeCounter.begin() ...)
        if kf_bad[s]:                                                             # if(pKF->isBad()) continue;
            continue
        local.add(s)                                                              # local_key_frames.insert(pKF);

    def after(cur):                                                               # ++itKF on a std::set that may have grown: the next larger element
        later = [x for x in local if x > cur]
        return min(later) if later else None

    it = min(local) if local else None                                            # itKF = local_key_frames.begin()
    while it is not None:                                                         # itKF != itEndKF
        if _exceeds(len(local), n_max):                                           # if(local_key_frames.size() > params.N_max_local_keyframes) break;
            break
        pKF = it
        row = [int(x) for x in neigh[pKF]] if len(neigh) else []
        vNeighs = [x for x in row[:n_neighbor] if x != -1]                        # getBestCovisibilityKeyFrames(pKF, N_neighbor_keyframes)
        for pNeighKF in vNeighs:
            if not kf_bad[pNeighKF]:                                              # if(!pNeighKF->isBad())
                local.add(pNeighKF)
                break
        pParent = int(parent[pKF])                                                # pKF->GetParent()
        if pParent != -1:                                                         # if(pParent)
            local.add(pParent)
            break                                                                 # leaves the OUTER loop (:153)
        it = after(it)
    return local


def local_keyframes_fast(weights, kf_bad, neigh, parent, n_max, n_neighbor):
    """the same on a boolean array: -> (local uint8 [n_kf], n_local)"""
    w, bad = np.asarray(weights), np.asarray(kf_bad) != 0
    n_kf = len(w)
    local = (w > 0) & ~bad
    neigh = np.asarray(neigh, np.int64).reshape(n_kf, -1)
    cur = -1
    while True:
        rest = np.nonzero(local[cur + 1:])[0]
        if len(rest) == 0:
            break
        cur = cur + 1 + int(rest[0])
        if _exceeds(int(local.sum()), n_max):
            break
        row = neigh[cur, :n_neighbor]
        row = row[row >= 0]
        good = row[~bad[row]]
        if len(good):
            local[good[0]] = True
        if parent[cur] >= 0:
            local[parent[cur]] = True
            break
    return local.astype(np.uint8), int(local.sum())


def key_frame_matches(T):
    """KeyFrame::GetMapPointMatches() of every slot, built from the landmarks' observations (symmetric associations): a list per slot, in landmark
    order, with a None in front of every third entry — a key point without a landmark"""
    n_kf, off, kf = len(T["kf_id"]), T["lm_obs_offsets"], T["lm_obs_kf"]
    out = [[] for _ in range(n_kf)]
    for lm in range(len(off) - 1):
        for j in range(int(off[lm]), int(off[lm + 1])):
            s = int(kf[j])
            if len(out[s]) % 3 == 0:
                out[s].append(None)
            out[s].append(lm)
    return out


def local_points_literal(matches, lm_bad, local, frame_lm):
    """matches: key_frame_matches(); local: the set of slots; frame_lm: the frame's LandMarkMatches as a list indexed by LMid, -1 = nullptr.
    -> (sorted list of local_map_points handed to SearchByProjection, list of the LMids removeLandMarkAssociation is called on)"""
    local_map_points = set()                                                      # local_map_points.clear()
    for pKF in sorted(local):                                                     # for(itKF = local_key_frames.begin() ...)
        for pMP in matches[pKF]:                                                  # vpMPs = pKF->GetMapPointMatches()
            if pMP is None:                                                       # if(!pMP){continue;}
                continue
            if not lm_bad[pMP]:                                                   # if(!pMP->isBad())
                local_map_points.add(pMP)
    removed = []
    for LMid, pMP in enumerate(frame_lm):                                         # SearchLocalPoints: for(it = matches.cbegin() ...)
        pMP = int(pMP)
        if pMP == -1:
            continue
        if lm_bad[pMP]:
            removed.append(LMid)                                                  # pcurrent_frame->removeLandMarkAssociation(LMid);
        else:
            local_map_points.discard(pMP)                                         # local_map_points.erase(pMP);
    return sorted(local_map_points), removed                                      # v_lmp(local_map_points.begin(), local_map_points.end())


def pack_points(selected, removed, n_assoc, cap):
    """the literal version's lists in the layout of hs_local_points"""
    sel = np.full(cap, -1, np.int32)
    k = min(len(selected), cap)
    sel[:k] = selected[:k]
    rem = np.zeros(n_assoc, np.uint8)
    rem[removed] = 1
    return dict(frame_remove=rem, sel=sel, n_sel=len(selected))


def local_points_fast(T, local, frame_lm, cap):
    """from the table: -> dict(frame_remove uint8 [n_assoc], sel int32 [cap], n_sel)"""
    off, kf = np.asarray(T["lm_obs_offsets"]), np.asarray(T["lm_obs_kf"], np.int64)
    L, bad = len(off) - 1, np.asarray(T["lm_bad"]) != 0
    local = np.asarray(local) != 0
    owner = np.repeat(np.arange(L), np.diff(off))
    kf = kf[int(off[0]):int(off[-1])]
    inside = (kf >= 0) & (kf < len(local))
    hit = np.zeros(len(kf), bool)
    hit[inside] = local[kf[inside]]
    seen = np.bincount(owner[hit], minlength=L) > 0
    flm = np.asarray(frame_lm, np.int64).reshape(-1)
    valid = (flm >= 0) & (flm < L)
    rem = np.zeros(len(flm), np.uint8)
    rem[valid] = bad[flm[valid]]
    held = np.zeros(L, bool)
    held[flm[valid][~bad[flm[valid]]]] = True
    selected = np.nonzero(~bad & seen & ~held)[0]
    out = pack_points(selected.tolist(), [], len(flm), cap)
    out["frame_remove"] = rem
    return out


def gather(lms, sel, n_sel, cap):
    """hs_landmark_gather_device: records sel[j] with assoc_kp = -1 and skip = 0; past n_sel empty records with assoc_kp = -1 and skip = 1"""
    out = np.zeros(cap, lms.dtype)
    n = min(n_sel, cap)
    out[:n] = lms[sel[:n]]
    out["assoc_kp"] = -1
    out["skip"][:n] = 0
    out["skip"][n:] = 1
    return out


POINT_KEYS = ("frame_remove", "sel", "n_sel")


def same(got, want, keys=POINT_KEYS):
    for k in keys:
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            return k
    return None
