"""Downscaled inference on the device (anh_infer_scaled and its mirrors): read_sample's bilinear shrink (annonet.cpp:153), the
tiled annonet_infer() and resize_label_image (annonet_infer_main.cpp:413, annonet.cpp:132-141) in one call, against the numpy
restatements of the two resizes (tests/resize_util.py, tests/png_util.py) around the oracle's annonet_infer().  The feature is
integer-valued end to end: every comparison is equality (the one exception is the sharded path's known near-tie cap)."""
import os
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu
import resize_util as ru
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "annonet_amd", "lib", "annonet_infer_hip")
K = 3
OV = 35   # TrainingNet::GetRequiredInputDimension() of a 2-level net
SIZES = [(150, 170), (97, 131), (260, 190)]
FACTORS = [1.5, 2.0, 3.7]


def tp():
    return aa.tiling.parameters(96, 96, OV, OV)


@pytest.fixture(scope="module")
def nets():
    o = OracleNet(2, 3, K, 0.25, 4)
    p, r = random_params(o, 21)
    o.params[:], o.running[:] = p, r
    net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    net.set_params(p, r)
    return o, net, (p, r)


def image_of(shape, seed=4):
    return np.random.default_rng(seed + shape[0]).integers(0, 256, shape + (3,), dtype=np.uint8)


def oracle_scaled(o, img, factor, gains=None, detection_levels=None):
    """(original-size map, map at the net's resolution, planes at the net's resolution) as the reference's program computes them"""
    small = ru.shrink(img, factor)
    scaled, planes = o.infer(small, gains=gains, detection_levels=detection_levels, max_tile=(96, 96), overlap=OV, want_blended=True)
    return pu.resize_nearest(scaled, img.shape[1], img.shape[0]), scaled, planes


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape,scale", ru.CASES + [((4097, 3001), 1 / 2.37)])
def test_resize_image_kernel_equals_numpy(shape, scale, channels):
    rng = np.random.default_rng(shape[0] + 7 * shape[1] + channels)
    img = rng.integers(0, 256, shape + (channels,), dtype=np.uint8)
    out_h, out_w = ru.scaled_size(shape[0], scale), ru.scaled_size(shape[1], scale)
    want = ru.bilinear_to(img, out_h, out_w)
    for garbage in (0xAB, 0x00):   # a destination element the kernel leaves out keeps one of the two fills
        np.testing.assert_array_equal(aa.resize_image(img, out_h, out_w, prefill=garbage), want)
    if channels == 1:
        np.testing.assert_array_equal(aa.resize_image(img[:, :, 0], out_h, out_w, prefill=0x5C), want[:, :, 0])


@pytest.mark.parametrize("shape,scale", ru.CASES + [((4097, 3001), 1 / 2.37)])
def test_resize_labels_kernel_equals_numpy(shape, scale):
    # the direction inference uses: a map at the net's resolution blown up to `shape`; and the reverse
    rng = np.random.default_rng(shape[0] * 3 + shape[1])
    small_shape = (ru.scaled_size(shape[0], scale), ru.scaled_size(shape[1], scale))
    for src_shape, dst_shape in ((small_shape, shape), (shape, small_shape)):
        lab = rng.integers(0, 7, src_shape).astype(np.uint16)
        lab[rng.random(src_shape) < 0.2] = 65535
        want = pu.resize_nearest(lab, dst_shape[1], dst_shape[0])
        for garbage in (0xAB, 0x00):
            np.testing.assert_array_equal(aa.resize_labels(lab, dst_shape[1], dst_shape[0], prefill=garbage), want)
        assert (want == 65535).any()


# ---- 2. anh_scaled_dims ---------------------------------------------------------------------------------------------------
def test_scaled_dims_table():
    for f in (1.0, 1.5, 2.0, 2.37, 3.7, 4.0, 0.5, 0.25):
        for h, w in SIZES + [(101, 7), (1, 1), (3, 90), (4097, 3001), (2, 5), (11, 13)]:
            want = (int(np.floor(h / f + 0.5)), int(np.floor(w / f + 0.5)))
            if min(want) < 1:
                continue
            assert aa.scaled_dims(h, w, f) == want, (h, w, f)
    assert aa.scaled_dims(101, 7, 2.0) == (51, 4)     # 50.5 and 3.5 round up (std::round)


# ---- 3. end to end, fp32 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gains", [None, [0.0, 0.1, 0.0]])
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("shape", SIZES)
def test_scaled_inference_equals_oracle(nets, shape, factor, gains):
    o, net, _ = nets
    img = image_of(shape)
    want, want_scaled, want_planes = oracle_scaled(o, img, factor, gains=gains)
    got, scaled, planes = aa.annonet_infer_scaled(net, img, factor, gains=gains, tiling_parameters=tp(), want_scaled=True, want_blended=True)
    assert got.shape == shape and scaled.shape == aa.scaled_dims(shape[0], shape[1], factor)
    np.testing.assert_array_equal(scaled, want_scaled)
    np.testing.assert_array_equal(got, want)
    assert planes.tobytes() == want_planes.tobytes()
    np.testing.assert_array_equal(aa.annonet_infer_scaled(net, img, factor, gains=gains, tiling_parameters=tp()), want)


def test_scaled_inference_with_detection_levels(nets):
    o, net, _ = nets
    img = image_of((150, 170))
    det = [0.0, 5.0, 5.0]
    want, want_scaled, _ = oracle_scaled(o, img, 2.0, detection_levels=det)
    plain, _, _ = oracle_scaled(o, img, 2.0)
    assert (want != plain).any()        # the filter changes something at these levels
    got, scaled = aa.annonet_infer_scaled(net, img, 2.0, detection_levels=det, tiling_parameters=tp(), want_scaled=True)
    np.testing.assert_array_equal(scaled, want_scaled)
    np.testing.assert_array_equal(got, want)


# ---- 4. factor 1 ------------------------------------------------------------------------------------------------------------
def test_factor_one_is_annonet_infer(nets):
    _, net, _ = nets
    img = image_of((150, 170))
    labels, planes = aa.annonet_infer(net, img, tiling_parameters=tp(), want_blended=True)
    got, scaled, got_planes = aa.annonet_infer_scaled(net, img, 1.0, tiling_parameters=tp(), want_scaled=True, want_blended=True)
    np.testing.assert_array_equal(got, labels)
    np.testing.assert_array_equal(scaled, labels)
    assert got_planes.tobytes() == planes.tobytes()
    np.testing.assert_array_equal(aa.annonet_infer_scaled(net, img, 1.0, tiling_parameters=tp()), aa.annonet_infer(net, img, tiling_parameters=tp()))


# ---- 5. bf16 ------------------------------------------------------------------------------------------------------------------
def test_bf16_scaled_equals_plain_on_the_shrunk_image(nets):
    _, _, (p, r) = nets
    net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_BF16))
    net.set_params(p, r)
    for shape, factor in (((260, 190), 2.0), ((150, 170), 1.5)):
        img = image_of(shape)
        small = ru.shrink(img, factor)
        first = aa.annonet_infer(net, small, tiling_parameters=tp())
        second = aa.annonet_infer(net, small, tiling_parameters=tp())
        np.testing.assert_array_equal(first, second)       # run-to-run variation is not an excuse below
        got, scaled = aa.annonet_infer_scaled(net, img, factor, tiling_parameters=tp(), want_scaled=True)
        np.testing.assert_array_equal(scaled, first)
        np.testing.assert_array_equal(got, pu.resize_nearest(first, shape[1], shape[0]))


# ---- 6. dirty buffers, changing sizes ---------------------------------------------------------------------------------------------
def test_one_handle_changing_sizes(nets):
    o, _, (p, r) = nets
    net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    net.set_params(p, r)
    big, small = image_of((260, 190)), image_of((97, 131))
    first = aa.annonet_infer_scaled(net, big, 2.0, tiling_parameters=tp(), want_scaled=True)
    middle = aa.annonet_infer_scaled(net, small, 3.7, tiling_parameters=tp(), want_scaled=True)
    again = aa.annonet_infer_scaled(net, big, 2.0, tiling_parameters=tp(), want_scaled=True)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    for got, (img, f) in ((first, (big, 2.0)), (middle, (small, 3.7))):
        want, want_scaled, _ = oracle_scaled(o, img, f)
        np.testing.assert_array_equal(got[0], want)
        np.testing.assert_array_equal(got[1], want_scaled)


# ---- 7. two replicas ----------------------------------------------------------------------------------------------------------
def test_two_replicas(nets):
    _, one, (p, r) = nets
    img = image_of((260, 190))
    aa.set_devices([0, 0])
    try:
        net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    finally:
        aa.set_devices([])
    assert net.L.anh_handle_replicas(net.h, 0) == 2
    net.set_params(p, r)
    small = ru.shrink(img, 2.0)
    plain = aa.annonet_infer(net, small, tiling_parameters=tp())
    got, scaled = aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp(), want_scaled=True)
    np.testing.assert_array_equal(scaled, plain)
    np.testing.assert_array_equal(got, pu.resize_nearest(plain, img.shape[1], img.shape[0]))
    np.testing.assert_array_equal(aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp()), got)   # without scaled_labels: the merged map is the library's own
    single = aa.annonet_infer_scaled(one, img, 2.0, tiling_parameters=tp())
    assert (got != single).mean() < 1e-4     # equal except exact near-ties where four tiles meet


# ---- 8. device-resident form --------------------------------------------------------------------------------------------------
def test_device_resident_form(nets):
    import torch
    _, net, _ = nets
    img = image_of((150, 170))
    H, W = img.shape[:2]
    sh, sw = aa.scaled_dims(H, W, 2.0)
    want, want_scaled, want_planes = aa.annonet_infer_scaled(net, img, 2.0, gains=[0.0, 0.1, 0.0], tiling_parameters=tp(), want_scaled=True, want_blended=True)
    stream = torch.cuda.ExternalStream(net.stream_ptr())
    with torch.cuda.stream(stream):
        d_img = torch.from_numpy(img).cuda()
        d_labels = torch.full((H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        d_scaled = torch.full((sh * sw * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        d_planes = torch.full((K, sh, sw), float("nan"), dtype=torch.float32, device="cuda")
        aa.annonet_infer_scaled_device(net, d_img.data_ptr(), H, W, 2.0, d_labels.data_ptr(), d_scaled.data_ptr(), d_planes.data_ptr(), gains=[0.0, 0.1, 0.0], tiling_parameters=tp())
        d_only = torch.full((H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        aa.annonet_infer_scaled_device(net, d_img.data_ptr(), H, W, 2.0, d_only.data_ptr(), gains=[0.0, 0.1, 0.0], tiling_parameters=tp())
        stream.synchronize()
    np.testing.assert_array_equal(d_labels.cpu().numpy().view(np.uint16).reshape(H, W), want)
    np.testing.assert_array_equal(d_scaled.cpu().numpy().view(np.uint16).reshape(sh, sw), want_scaled)
    assert d_planes.cpu().numpy().tobytes() == want_planes.tobytes()
    np.testing.assert_array_equal(d_only.cpu().numpy().view(np.uint16).reshape(H, W), want)


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,needle", [(0.0, "positive finite"), (-2.0, "positive finite"), (float("nan"), "positive finite"), (float("inf"), "positive finite"),
                                           (400.0, "too small for this downscaling factor"), (1e-3, "beyond 32768")])
def test_bad_factors_are_errors(nets, factor, needle):
    _, net, _ = nets
    img = image_of((150, 170))
    with pytest.raises(aa.AnnonetHipError, match=needle) as e:
        aa.annonet_infer_scaled(net, img, factor, tiling_parameters=tp())
    assert "downscaling factor" in str(e.value)
    with pytest.raises(aa.AnnonetHipError, match=needle):
        aa.scaled_dims(150, 170, factor)
    np.testing.assert_array_equal(aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp()), aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp()))   # the handle is still usable


# ---- 10. the inference program ----------------------------------------------------------------------------------------------
def parse_matrix(lines, at):
    rows = []
    for line in lines[at + 3:at + 3 + K]:
        toks = [t for t in line.split() if t != "truth"]
        rows.append([int(v) for v in toks[1:1 + K]])
    return np.array(rows)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, nets):
    _, net, _ = nets
    d = tmp_path_factory.mktemp("anno_scaled")
    (d / "annonet.dnn").write_bytes(aa.dnn_envelope_pack("", 2.0, net.Serialize()))
    rng = np.random.default_rng(5)
    images = {}
    (d / "sub").mkdir()
    for name, (h, w), with_mask in (("a.png", (150, 170), True), ("sub/b.png", (97, 131), True), ("c.png", (260, 190), False)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pu.write_png(d / name, img, filter_type=1)
        gt = None
        if with_mask:   # at the ORIGINAL size: the program resizes it to the net's resolution (annonet.cpp:160-166)
            gt = np.zeros((h, w), np.uint16)
            for _ in range(10):
                y, x = rng.integers(0, h), rng.integers(0, w)
                gt[y:y + rng.integers(5, 40), x:x + rng.integers(5, 40)] = rng.integers(0, K)
            gt[rng.random((h, w)) < 0.3] = 65535
            pu.write_png(str(d / name) + "_mask.png", pu.labels_to_rgba(gt))
        images[name] = (img, gt)
    return d, images


def run_tool(d, *extra):
    r = subprocess.run([TOOL, str(d), "--dnn", str(d / "annonet.dnn"), "-w", "96", "-h", "96", "--precision", "fp32", *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_infer_program_with_a_downscaled_net(dataset, nets):
    o = nets[0]
    d, images = dataset
    out = run_tool(d)
    assert "Deserializing annonet, downscaling factor = 2" in out
    assert "All result images written!" in out
    per_pixel, per_region = np.zeros((K, K), np.int64), np.zeros((K, K), np.int64)
    pngs = {}
    for name, (img, gt) in images.items():
        want, want_scaled, _ = oracle_scaled(o, img, 2.0)
        pngs[name] = open(str(d / name) + "_result.png", "rb").read()
        got = pu.read_png(str(d / name) + "_result.png")
        assert got.shape[:2] == img.shape[:2]
        np.testing.assert_array_equal(got, pu.labels_to_rgba(want))
        if gt is not None:
            pp, pr = pu.confusion_matrices(pu.resize_nearest(gt, want_scaled.shape[1], want_scaled.shape[0]), want_scaled, K)
            per_pixel += pp
            per_region += pr

    def matrices(text):
        lines = text.splitlines()
        return parse_matrix(lines, lines.index("Confusion matrix per pixel:")), parse_matrix(lines, lines.index("Confusion matrix per region (two-way):"))
    got_pixel, got_region = matrices(out)
    np.testing.assert_array_equal(got_pixel, per_pixel)
    np.testing.assert_array_equal(got_region, per_region)
    assert per_pixel.sum() > 1000 and per_region.sum() > 10
    for name in images:
        os.remove(str(d / name) + "_result.png")
    out = run_tool(d, "--host-resize")       # the reference's placement of the two resizes: same files, same matrices
    assert "Deserializing annonet, downscaling factor = 2" in out
    for name in images:
        assert open(str(d / name) + "_result.png", "rb").read() == pngs[name]
    host_pixel, host_region = matrices(out)
    np.testing.assert_array_equal(host_pixel, per_pixel)
    np.testing.assert_array_equal(host_region, per_region)


# ---- 11. the C++ drop-in header ---------------------------------------------------------------------------------------------------
def test_cpp_header_annonet_infer_scaled(tmp_path, nets):
    _, net, _ = nets
    exe = str(tmp_path / "scaled_infer_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "scaled_infer_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    img = image_of((150, 170))
    (tmp_path / "net.bin").write_bytes(net.Serialize())
    (tmp_path / "image.raw").write_bytes(img.tobytes())
    r = subprocess.run([exe, str(tmp_path / "net.bin"), str(tmp_path / "image.raw"), "150", "170", "2", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want, want_scaled, want_planes = aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp(), want_scaled=True, want_blended=True)
    sh, sw = want_scaled.shape
    assert r.stdout.split() == ["150", "170", str(sh), str(sw), str(K)]
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.labels.raw").read_bytes(), np.uint16).reshape(150, 170), want)
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.scaled.raw").read_bytes(), np.uint16).reshape(sh, sw), want_scaled)
    assert (tmp_path / "out.planes.raw").read_bytes() == want_planes.tobytes()
