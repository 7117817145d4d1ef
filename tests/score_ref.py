"""Reference for the device's scoring of a result label map against its ground truth (anh_score_device and its forms).

The rule (annonet_hip.h states it; annonet_amd/host/annonet_host.h: RegionScorer and the per-pixel loop of the inference tool are its
origin).  truth and result are u16 maps of one size, K the class count.  A pixel is LABELLED where truth < K; a prediction >= K casts
no vote.

  labelled      the number of labelled pixels
  pixel[t][p]   labelled pixels with truth == t and result == p < K
  region[t][p]  for each map M of (truth, result): the regions of M are its blobs (blobs_ref) plus region 0 = all pixels where M == 0.
                T[c] / P[c] = the region's labelled pixels with truth == c / result == c < K.  No vote where T is all zero; t = first
                index of max(T); bg_only = P[0] > 0 and nothing else in P; where t != 0 and not bg_only P[0] = 0; no vote where P is
                all zero; else region[t][first index of max(P)] += 1.

score_ref is that rule in numpy; score_literal transcribes RegionScorer and the tool's per-pixel loop line by line, for small maps."""
import numpy as np

import blobs_ref

IGNORE = 65535


def score_ref(truth, result, K):
    """(pixel [K,K] u64, region [K,K] u64, labelled)"""
    truth = np.asarray(truth).astype(np.int64)
    result = np.asarray(result).astype(np.int64)
    assert truth.shape == result.shape and truth.ndim == 2
    lab = truth < K
    votes = lab & (result < K)
    pixel = np.zeros((K, K), np.uint64)
    np.add.at(pixel, (truth[votes], result[votes]), 1)
    region = np.zeros((K, K), np.uint64)
    for M in (truth, result):
        blobs, count = blobs_ref.blobs_ref(M.astype(np.uint16))      # blob 0 = the background: region 0
        reg = blobs.astype(np.int64)
        T = np.zeros((count, K), np.int64)
        P = np.zeros((count, K), np.int64)
        np.add.at(T, (reg[lab], truth[lab]), 1)
        np.add.at(P, (reg[votes], result[votes]), 1)
        t = T.argmax(axis=1)                                         # argmax: the first index of the maximum
        bg_only = (P[:, 0] > 0) & (P[:, 1:].sum(axis=1) == 0)
        P[(t != 0) & ~bg_only, 0] = 0
        ok = (T.sum(axis=1) > 0) & (P.sum(axis=1) > 0)
        np.add.at(region, (t[ok], P.argmax(axis=1)[ok]), 1)
    return pixel, region, int(lab.sum())


def score_ref_batch(truths, results, K):
    """the three outputs of the batched calls: pixel [n,K,K], region [n,K,K], labelled [n]"""
    out = [score_ref(t, r, K) for t, r in zip(truths, results)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.uint64))


class _Tally:
    """RegionScorer::Tally: votes per class"""

    def __init__(self):
        self.by_class = {}

    def add(self, cls):
        self.by_class[cls] = self.by_class.get(cls, 0) + 1

    def winner(self):
        best, most = IGNORE, 0
        for c in sorted(self.by_class):          # ascending class index: a tie stays with the smaller one
            if self.by_class[c] > most:
                most, best = self.by_class[c], c
        return best

    def distinct(self):
        return sum(1 for v in self.by_class.values() if v > 0)


def score_literal(truth, result, K):
    """The tool's `score` lambda and RegionScorer::score / vote, line by line: labeled_points_by_class as decode_rgba_label_image fills
    it (here: every truth value below K; mask decoding produces no other value but 65535), dict tallies, label_connected_blobs as
    blobs_ref.flood_fill.  Like the scorer it tallies every prediction but 65535; result maps hold no other value >= K."""
    truth = np.asarray(truth)
    result = np.asarray(result)
    nr, nc = truth.shape
    points = {}
    for r in range(nr):
        for c in range(nc):
            label = int(truth[r, c])
            if label < K:
                points.setdefault(label, []).append((c, r))          # dlib::point(x, y)
    pixel = np.zeros((K, K), np.uint64)
    region = np.zeros((K, K), np.uint64)
    labelled = 0

    def add(matrix, t, p):                                           # ConfusionMatrix::add
        if t < K and p < K:
            matrix[t, p] += 1

    for cls in sorted(points):
        for (x, y) in points[cls]:
            add(pixel, cls, int(result[y, x]))
        labelled += len(points[cls])
    if not points:
        return pixel, region, labelled
    for M in (truth, result):
        region_of, regions = blobs_ref.flood_fill(M)
        in_truth = [_Tally() for _ in range(regions)]
        in_result = [_Tally() for _ in range(regions)]
        for cls in sorted(points):
            for (x, y) in points[cls]:
                reg = int(region_of[y, x])
                in_truth[reg].add(cls)
                predicted = int(result[y, x])
                if predicted != IGNORE:
                    in_result[reg].add(predicted)
        for r in range(regions):
            truth_class = in_truth[r].winner()
            if truth_class == IGNORE:
                continue
            predicted = in_result[r]
            background_only = predicted.distinct() == 1 and predicted.by_class.get(0, 0) > 0
            if truth_class != 0 and not background_only and predicted.by_class:
                predicted.by_class[0] = 0
            add(region, truth_class, predicted.winner())
    return pixel, region, labelled


# ---- the hand-worked cases (K = 3): truth, result, cells of pixel, cells of region, labelled; unlisted cells are 0 ----
HAND_K = 3
HAND_CASES = {
    "defect_truth_drops_background_votes": ([[2, 2, 2, 2]], [[0, 0, 0, 1]], {(2, 0): 3, (2, 1): 1}, {(2, 1): 2, (2, 0): 1}, 4),
    "tie_goes_to_the_smaller_class": ([[1, 1, 1, 1]], [[2, 2, 1, 1]], {(1, 1): 2, (1, 2): 2}, {(1, 1): 2, (1, 2): 1}, 4),
    "truth_all_ignore": ([[IGNORE] * 4], [[0, 1, 2, 1]], {}, {}, 0),
    "result_all_nan": ([[0, 1, 2, 2]], [[IGNORE] * 4], {}, {}, 4),
}


def hand_case(name):
    """(truth u16, result u16, pixel [3,3], region [3,3], labelled)"""
    truth, result, pixel_cells, region_cells, labelled = HAND_CASES[name]
    pixel = np.zeros((HAND_K, HAND_K), np.uint64)
    region = np.zeros((HAND_K, HAND_K), np.uint64)
    for (t, p), v in pixel_cells.items():
        pixel[t, p] = v
    for (t, p), v in region_cells.items():
        region[t, p] = v
    return np.array(truth, np.uint16), np.array(result, np.uint16), pixel, region, labelled


def result_for(truth_name, shape, which):
    """the result map that goes with a truth pattern in the device tests: the next pattern of blobs_ref.PATTERNS, the pattern with
    65535 and values >= K, or a smooth map"""
    if which == "next":
        names = blobs_ref.PATTERNS
        return blobs_ref.pattern(names[(names.index(truth_name) + 1) % len(names)], shape)
    if which == "wide":
        return np.flipud(blobs_ref.pattern("random_wide_values", shape)).copy()     # (flipped: not the truth map itself when that is the truth)
    if which == "smooth":
        return blobs_ref.smooth_map(shape, 11 + shape[0] + shape[1])
    raise KeyError(which)
