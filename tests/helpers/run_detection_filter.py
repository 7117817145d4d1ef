"""The detection filter on the maps of detection_filter_ref.REFERENCE_ORDER_MAPS in a fresh process (ANH_DET_SEED_REFERENCE_ORDER is an
environment switch read once per process), on ONE handle after a larger call that leaves its scratch dirty: writes the filtered maps.
usage: run_detection_filter.py out.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import annonet_amd as aa  # noqa: E402
import detection_filter_ref as dr  # noqa: E402

net = aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))
big = dr.pattern("random", (200, 300))
planes, levels = dr.plan("random", big, "random")
aa.detection_filter(big, planes, levels, net=net, prefill_scratch=True)
res = {}
for name, shape in dr.REFERENCE_ORDER_MAPS:
    lab = dr.pattern(name, shape)
    planes, levels = dr.plan("random", lab, name)
    res["%s_%dx%d" % ((name,) + shape)], _ = aa.detection_filter(lab, planes, levels, net=net)
np.savez(sys.argv[1], **res)
