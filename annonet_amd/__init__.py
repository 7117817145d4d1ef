"""annonet_amd — MI355X-native (gfx950) implementation of annonet's hot path: the segmentation net's training step and
tiled sliding-window inference, behind the reference's NetPimpl / tiling / annonet_infer interface.

The compute lives in annonet_amd/lib/libannonet_hip.so (hand-written HIP, C ABI in include/annonet_hip.h); this package
is the thin host-side mirror used by tests and bench.py.  There is no CPU fallback.
"""
from ._lib import ANH_BF16, ANH_FP32, LABEL_IGNORE, AnnonetHipError, build, lib  # noqa: F401
from .netpimpl import (Dataset, RuntimeNet, TrainingNet, REGION_DTYPE, argmax_device, annonet_infer, annonet_infer_device, annonet_infer_regions, label_blobs, regions, regions_device, detection_filter, detection_filter_device, label_blobs_batch, regions_batch, regions_batch_device, annonet_infer_regions_batch, annonet_infer_regions_scaled, annonet_infer_regions_scaled_batch, annonet_infer_scaled, annonet_infer_scaled_device, annonet_infer_scaled_batch, annonet_infer_scaled_batch_device, annonet_infer_batch, annonet_infer_batch_device, infer_batch_plan, labels_from_logits_device, count_steps_without_decrease, dnn_envelope_pack, dnn_envelope_unpack,  # noqa: F401
                       ignore_large_nonzero_regions, score, score_batch, score_device, score_batch_device,
                       EVAL_DTYPE, EvalResult, eval_logits_device,
                       net_config, net_layers,
                       op_conv_backward_data, op_conv_backward_data_bn, op_conv_backward_filter, op_conv_backward_filter_bn,
                       op_conv_forward, op_conv_forward_stats, outpaint,
                       op_bn_backward, op_bn_fold, op_bn_forward_stats, op_conv_backward_data_bn_table, op_conv_forward_stats_table, op_head_train, op_loss,
                       random_rect_containing_point, resolve_pick, resize_image, resize_labels, resize_image_batch, resize_labels_batch, scaled_dims, set_devices, set_weights, shard_range, cross_replica_overlaps, tiling)
