"""axial_vs_amd -- MI355X-native axial-trajectory attention (Axial-VS / MaXTron hot path).

Python host mirroring the reference nn.Module surface; all compute runs in hand-written HIP kernels
behind the C-ABI of libaxvs.so (include/axvs.h).
"""
from .modules import (AxialTrajectoryAttention5D, PositionEmbeddingSine3D, TemporalAxialTrajectoryAttentionLayer,
                      GraphedForward, TemporalEncoder, TemporalTrajectoryAttentionLayer, TrajectoryAttention,
                      TubeLinkTemporalEncoder, disable_range_check, enable_range_check, invalidate_pack,
                      range_check_report, set_default_dtype, check_status, set_handoff_policy)

from .cross_clip import CrossClipTrackingModule, TubeLinkCrossClipHead
from .pixel_decoder import (MSDeformAttnPixelDecoder, MSDeformAttnTransformerEncoder, MSDeformAttnTransformerEncoderOnly,
                            PositionEmbeddingSine, WithinClipTrackingModule)
from .matching import VideoHungarianMatcher, linear_sum_assignment, match_clips, match_from_embds, match_layers, matcher_costs
from .criterion import MaXTronCCSetCriterion, MaXTronWCSetCriterion, draw_sampling_noise, sampled_pixel_losses, set_criterion_losses
from .tl_criterion import TubeLinkSetCriterion, draw_point_coords, tube_link_losses
from .panoptic import VideoPanopticPostProcessor, video_panoptic_inference
from .instances import VideoInstancePostProcessor, unpack_bits, video_instance_inference
from .tube_link import MultiScaleDeformableAxialTrajectoryAttention
from .tl_pixel_decoder import TubeLinkPixelDecoder
from .clip_decoder import TubeLinkClipDecoder, tube_link_clip_queries
from .kmax_decoder import KMaXTransformerDecoder, filter_training_keys, kmax_decoder_forward
from .kmax_pixel_decoder import KMaXPixelDecoder, MaXTronDeepLabHead, kmax_pixel_decoder_forward
from .convnext import ConvNeXtBackbone, ConvNeXtV2Backbone, convnext_forward
from .resnet import ResNetBackbone, resnet_forward
from .msda import MSDeformAttn, MSDeformAttnFunction, MSDeformAttnTransformerEncoderLayer, ms_deform_attn_backward, ms_deform_attn_forward

__all__ = ["video_panoptic_inference", "VideoPanopticPostProcessor", "video_instance_inference", "VideoInstancePostProcessor", "unpack_bits", "MultiScaleDeformableAxialTrajectoryAttention", "TubeLinkPixelDecoder", "TubeLinkClipDecoder", "tube_link_clip_queries", "KMaXTransformerDecoder", "kmax_decoder_forward", "filter_training_keys", "KMaXPixelDecoder", "kmax_pixel_decoder_forward", "MaXTronDeepLabHead", "ConvNeXtBackbone", "ConvNeXtV2Backbone", "convnext_forward", "ResNetBackbone", "resnet_forward", "linear_sum_assignment", "match_from_embds", "match_clips", "VideoHungarianMatcher", "match_layers", "matcher_costs", "MaXTronCCSetCriterion", "MaXTronWCSetCriterion", "set_criterion_losses", "draw_sampling_noise", "sampled_pixel_losses", "TubeLinkSetCriterion", "draw_point_coords", "tube_link_losses", "WithinClipTrackingModule", "MSDeformAttnPixelDecoder", "MSDeformAttnTransformerEncoder", "MSDeformAttnTransformerEncoderOnly",
           "PositionEmbeddingSine", "CrossClipTrackingModule", "TubeLinkCrossClipHead", "MSDeformAttn", "MSDeformAttnTransformerEncoderLayer", "ms_deform_attn_forward", "ms_deform_attn_backward", "MSDeformAttnFunction", "TrajectoryAttention", "TemporalAxialTrajectoryAttentionLayer", "TemporalTrajectoryAttentionLayer",
           "TemporalEncoder", "TubeLinkTemporalEncoder", "PositionEmbeddingSine3D", "AxialTrajectoryAttention5D",
           "set_default_dtype", "GraphedForward", "invalidate_pack", "enable_range_check", "range_check_report", "disable_range_check", "check_status", "set_handoff_policy"]
