"""Scoring on the device (anh_score_device, anh_score_batch_device, anh_score, anh_score_batch) against tests/score_ref.py: labelled
pixels, per-pixel counts and two-way per-region votes, exact integers.  The maps are those of the blob tests (blobs_ref.SIZES x PATTERNS):
regions across the 32-pixel tile seams, 97 x 130 spans four of the tally's 4096-pixel blocks, "random" crowds a block's LDS vote table
into the global fallback, "full" takes the wave-uniform path.  The result maps carry 65535 and values >= K; K is 2, 3 and 7.  Outputs
are prefilled with 0xFF where a stale element would show."""
import functools

import numpy as np
import pytest

import annonet_amd as aa
import blobs_ref as br
import score_ref as sr

pytestmark = pytest.mark.gpu

CLASSES = [2, 3, 7]
RESULTS = ["next", "wide", "smooth"]
INVALID = 1


@functools.lru_cache(maxsize=None)
def pair(truth_name, shape, which):
    truth, result = br.pattern(truth_name, shape), sr.result_for(truth_name, shape, which)
    truth.setflags(write=False)
    result.setflags(write=False)
    return truth, result


@functools.lru_cache(maxsize=None)
def expected(truth_name, shape, which, K):
    return sr.score_ref(*pair(truth_name, shape, which), K)


def assert_counts(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"pixel {what}")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"region {what}")
    np.testing.assert_array_equal(np.asarray(got[2], np.uint64), np.asarray(want[2], np.uint64), err_msg=f"labelled {what}")


def device_score(net, truth, result, K, prefill=0xFF):
    """anh_score_device on maps torch uploads"""
    import torch
    d_t = torch.from_numpy(np.array(truth, np.uint16).view(np.int16)).cuda()       # (a writable copy: the shared maps are read-only)
    d_r = torch.from_numpy(np.array(result, np.uint16).view(np.int16)).cuda()
    torch.cuda.current_stream().synchronize()      # the uploads ran on torch's stream; the scoring runs on the handle's
    return aa.score_device(net, d_t.data_ptr(), d_r.data_ptr(), K, truth.shape[0], truth.shape[1], prefill=prefill)


@pytest.fixture(scope="module")
def net():
    return aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))


@pytest.mark.parametrize("shape", br.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("truth_name", br.PATTERNS)
def test_counts_equal_the_reference(net, truth_name, shape):
    for which in RESULTS:
        truth, result = pair(truth_name, shape, which)
        for K in CLASSES:
            want = expected(truth_name, shape, which, K)
            assert_counts(device_score(net, truth, result, K), want, f"device form, {which}, K={K}")
            assert_counts(aa.score(truth, result, K, prefill=0xFF, net=net), want, f"host form, {which}, K={K}")


@pytest.mark.parametrize("K", [33, 40])
def test_class_counts_around_the_lds_matrix(net, K):
    """K * K <= 1024 keeps a block's per-pixel counts in LDS; K = 33 takes the global atomics"""
    rng = np.random.default_rng(K)
    truth = rng.integers(0, K + 2, (70, 67)).astype(np.uint16)
    result = rng.integers(0, K + 2, (70, 67)).astype(np.uint16)
    assert_counts(device_score(net, truth, result, K), sr.score_ref(truth, result, K))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(33, 31), (97, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_batch_equals_the_reference_and_the_single_calls(net, n, shape):
    import torch
    names = ["random", "smooth", "u_shape"][:n]
    truths = np.stack([br.smooth_map(shape, 5) if m == "smooth" else br.pattern(m, shape) for m in names])
    results = np.stack([sr.result_for("random", shape, w) for w in ["wide", "smooth", "next"][:n]])
    for K in CLASSES:
        want = sr.score_ref_batch(truths, results, K)
        got = aa.score_batch(truths, results, K, prefill=0xFF, net=net)
        assert_counts(got, want, f"host form, K={K}")
        d_t = torch.from_numpy(truths.view(np.int16)).cuda()
        d_r = torch.from_numpy(results.view(np.int16)).cuda()
        torch.cuda.current_stream().synchronize()
        got_d = aa.score_batch_device(net, d_t.data_ptr(), d_r.data_ptr(), n, K, shape[0], shape[1], prefill=0xFF)
        assert_counts(got_d, want, f"device form, K={K}")
        for i in range(n):       # image i of a batch equals the single-image call on that pair, bit for bit
            one = aa.score(truths[i], results[i], K, prefill=0xFF, net=net)
            assert_counts((got[0][i], got[1][i], got[2][i]), one, f"image {i}, K={K}")


def test_three_times_one_pair_gives_three_equal_blocks(net):
    truth, result = pair("random", (97, 130), "wide")
    pixel, region, labelled = aa.score_batch(np.stack([truth] * 3), np.stack([result] * 3), 3, prefill=0xFF, net=net)
    want = expected("random", (97, 130), "wide", 3)
    for i in range(3):
        assert_counts((pixel[i], region[i], labelled[i]), want, f"image {i}")


def test_a_small_call_after_a_large_one_reads_nothing_stale():
    """one handle of its own: the large call leaves vote rows, matrices and blob maps behind that the small one must not read"""
    own = aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))
    big_t, big_r = pair("random", (97, 130), "wide")
    assert_counts(aa.score(big_t, big_r, 7, prefill=0xFF, net=own), expected("random", (97, 130), "wide", 7), "large")
    small_t, small_r = pair("random", (1, 70), "smooth")
    assert_counts(aa.score(small_t, small_r, 2, prefill=0xFF, net=own), expected("random", (1, 70), "smooth", 2), "small after large")
    truth, result, pixel, region, labelled = sr.hand_case("defect_truth_drops_background_votes")
    assert_counts(aa.score(truth, result, sr.HAND_K, prefill=0xFF, net=own), (pixel, region, labelled), "1 x 4 after large")


@pytest.mark.parametrize("name", sorted(sr.HAND_CASES))
def test_hand_worked_cases(net, name):
    truth, result, pixel, region, labelled = sr.hand_case(name)
    assert truth.shape == (1, 4)
    assert_counts(device_score(net, truth, result, sr.HAND_K), (pixel, region, labelled))
    assert_counts(aa.score(truth, result, sr.HAND_K, prefill=0xFF, net=net), (pixel, region, labelled))


def test_any_output_may_be_null(net):
    import ctypes as C
    truth, result = pair("random", (33, 31), "wide")
    want = expected("random", (33, 31), "wide", 3)
    region = np.full((3, 3), 2**64 - 1, np.uint64)
    t, r = np.ascontiguousarray(truth), np.ascontiguousarray(result)
    aa._lib.check(net.L.anh_score(net.h, t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), 3, 33, 31, None, region.ctypes.data_as(C.c_void_p), None))
    np.testing.assert_array_equal(region, want[1])


def test_refusals_leave_the_handle_usable(net):
    import ctypes as C
    import torch
    truth, result = pair("random", (33, 31), "wide")
    d_t = torch.from_numpy(np.array(truth, np.uint16).view(np.int16)).cuda()
    d_r = torch.from_numpy(np.array(result, np.uint16).view(np.int16)).cuda()
    torch.cuda.current_stream().synchronize()
    out = [np.zeros(9, np.uint64), np.zeros(9, np.uint64), np.zeros(1, np.uint64)]
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in out]
    L = net.L
    assert L.anh_score_batch_device(net.h, d_t.data_ptr(), d_r.data_ptr(), 1, 0, 33, 31, *ptrs) == INVALID            # classes = 0
    assert L.anh_score_batch_device(net.h, None, d_r.data_ptr(), 1, 3, 33, 31, *ptrs) == INVALID                      # a null map, outputs given
    assert L.anh_score_batch_device(net.h, d_t.data_ptr(), None, 1, 3, 33, 31, *ptrs) == INVALID
    assert L.anh_score_batch_device(net.h, d_t.data_ptr(), d_r.data_ptr(), 0, 3, 33, 31, *ptrs) == INVALID            # n = 0
    with pytest.raises(aa.AnnonetHipError) as e:
        aa.score_device(net, d_t.data_ptr(), d_r.data_ptr(), 0, 33, 31)
    assert e.value.code == INVALID
    assert_counts(aa.score_device(net, d_t.data_ptr(), d_r.data_ptr(), 3, 33, 31, prefill=0xFF), expected("random", (33, 31), "wide", 3), "after the refusals")
