"""The scoring rule's two references agree (tests/score_ref.py): score_ref, the rule in numpy on blobs_ref, and score_literal, the
transcription of RegionScorer and the tool's per-pixel loop; and both give the hand-worked answers.  No device is touched."""
import numpy as np
import pytest

import blobs_ref as br
import score_ref as sr

SMALL = [(1, 1), (1, 9), (7, 1), (5, 6), (12, 11), (31, 33)]


def in_domain(result, K):
    """the scorer's own domain: a result value is a class or 65535 (the rule drops every value >= K, the scorer only 65535)"""
    out = np.asarray(result).copy()
    out[out >= K] = sr.IGNORE
    return out


def assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0], err_msg="pixel")
    np.testing.assert_array_equal(a[1], b[1], err_msg="region")
    assert a[2] == b[2]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("truth_name", br.PATTERNS)
@pytest.mark.parametrize("K", [2, 3, 7])
def test_rule_and_transcription_agree(shape, truth_name, K):
    truth = br.pattern(truth_name, shape)
    for which in ("next", "wide", "smooth"):
        result = in_domain(sr.result_for(truth_name, shape, which), K)
        assert_same(sr.score_ref(truth, result, K), sr.score_literal(truth, result, K))


@pytest.mark.parametrize("seed", range(8))
def test_rule_and_transcription_agree_on_noise(seed):
    rng = np.random.default_rng(seed)
    K = (2, 3, 7)[seed % 3]
    values = np.array(list(range(K)) + [sr.IGNORE], np.uint16)
    truth = rng.choice(values, size=(9, 13))
    result = rng.choice(values, size=(9, 13))
    assert_same(sr.score_ref(truth, result, K), sr.score_literal(truth, result, K))


def test_a_prediction_of_no_class_is_dropped_by_the_rule():
    """7 is no class when K = 3: the rule counts the remaining votes, so the region still votes for 1"""
    truth = np.array([[1, 1, 1]], np.uint16)
    result = np.array([[7, 7, 1]], np.uint16)
    pixel, region, labelled = sr.score_ref(truth, result, 3)
    assert labelled == 3 and pixel[1, 1] == 1 and pixel.sum() == 1
    assert region[1, 1] == 2 and region.sum() == 2          # the truth blob, and the result blob of label 1; the blob of 7 predicts nothing


@pytest.mark.parametrize("name", sorted(sr.HAND_CASES))
@pytest.mark.parametrize("fn", [sr.score_ref, sr.score_literal], ids=["rule", "transcription"])
def test_hand_worked_cases(name, fn):
    truth, result, pixel, region, labelled = sr.hand_case(name)
    assert_same(fn(truth, result, sr.HAND_K), (pixel, region, labelled))
    if name == "result_all_nan":
        assert labelled > 0
