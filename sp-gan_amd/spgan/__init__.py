"""spgan: MI355X-native SP-GAN train-step hot path (HIP kernels behind the reference's nn.Module surface).

    from spgan import Generator, Discriminator, EdgeBlock, AdaptivePointNorm, get_edge_features
    from spgan import dis_loss, gen_loss, GradientPenalty, TrainStep

Importing the package does not touch the GPU; the shared library is loaded on first use and its
absence is a hard error (there is no CPU fallback).
"""
from . import block_tail, dataset, edge_conv, edge_max, edge_rank, edge_weight, edge_window, fixture_rng, metrics, ops, pointconv_util, pointnet_util, point_attn, gc_attn, sampling  # noqa: F401
from . import approxmatch, augment, compat, fpd, pointops                  # noqa: F401
from .augment import BatchAugment                                          # noqa: F401
from .approxmatch import MatchCostFunction, approx_match, emd_approx_match, match_cost, match_cost_dense   # noqa: F401
from . import pointnet2_modules, pointnet2_utils, pytorch_utils            # noqa: F401
from .capture import CapturedBody                                          # noqa: F401
from .losses import GradientPenalty, dis_loss, gen_loss                    # noqa: F401
from .modules import (AdaptivePointNorm, Discriminator, EdgeBlock, Generator, bilateral_upsample_edgeConv, conv2dbr, deform_edgeConv,   # noqa: F401
                      deform_edgeConv_feat, deform_edgeConv_first, deform_edgeConv_simple, edgeConv, get_edge_features, get_edge_features_xyz, upsample_edgeConv)
from .modules import (bilateral_block, bilateral_block_l1, bilateral_block_l2, bilateral_block_l3, bilateral_block_l4, deform_block_feat,   # noqa: F401
                      deform_block_feat_middle, deform_block_middle, deform_block_tail)
from .modules import Attention, PointTransformerLayer, Self_Attn            # noqa: F401
from .modules import Dense_Attn, DenseEdgeModule, DenseModule1D, get_graph_feature            # noqa: F401
from .modules import Dense_Attn_2D, DenseModule2D, GC_attn, MultiDenseMLP, Self_Attn2                                        # noqa: F401
from . import gan_layers                                                    # noqa: F401
from .gan_layers import (AdaptiveInstanceNorm, LayerEpilogue, MinibatchStdDev, NoiseInjection, NoiseLayer, PixelNorm, PixelwiseNorm,   # noqa: F401
                         SpectralNorm, StddevLayer, Truncation, WScaleLayer, l2normalize, snconv2d, snlinear, spectral_norm,
                         spectral_norm_network)
from .expansion_penalty import expansionPenaltyFunction, expansionPenaltyModule   # noqa: F401
from .mds import gather_operation, minimum_density_sample                       # noqa: F401
from . import model_utils                                                       # noqa: F401
from .model_utils import (get_cd_loss, get_cd_loss2, get_emd_loss, get_hausdorff_loss, get_perulsion_loss, get_repulsion_loss,   # noqa: F401
                          get_repulsion_loss4, get_uniform_loss_knn, group_nearest)
from .optim import EMA, Adam, StepLR, flatten_module                       # noqa: F401
from .parallel import DataParallel, init_process_group_from_env, shard_batch   # noqa: F401
from .train import TrainStep, requires_grad                                # noqa: F401

__all__ = ["Generator", "Discriminator", "EdgeBlock", "AdaptivePointNorm", "get_edge_features", "edgeConv", "conv2dbr", "upsample_edgeConv", "get_edge_features_xyz", "deform_edgeConv_simple",
           "deform_edgeConv_first", "deform_edgeConv_feat", "deform_edgeConv", "bilateral_upsample_edgeConv", "bilateral_block", "bilateral_block_l1",
           "bilateral_block_l2", "bilateral_block_l3", "bilateral_block_l4", "deform_block_middle", "deform_block_tail", "deform_block_feat_middle",
           "deform_block_feat", "PointTransformerLayer", "Attention", "Self_Attn", "Self_Attn2", "DenseEdgeModule", "DenseModule1D", "Dense_Attn", "GC_attn", "DenseModule2D", "MultiDenseMLP", "Dense_Attn_2D", "get_graph_feature", "dis_loss", "gen_loss",
           "expansionPenaltyFunction", "expansionPenaltyModule", "minimum_density_sample", "gather_operation",
           "GradientPenalty", "TrainStep", "CapturedBody", "Adam", "EMA", "StepLR", "DataParallel", "requires_grad", "ops", "fixture_rng", "sampling", "pointops", "compat", "fpd",
           "pointnet2_utils", "pointnet2_modules", "pytorch_utils",
           "gan_layers", "SpectralNorm", "spectral_norm", "spectral_norm_network", "snconv2d", "snlinear", "l2normalize", "MinibatchStdDev",
           "StddevLayer", "PixelNorm", "PixelwiseNorm", "NoiseLayer", "NoiseInjection", "LayerEpilogue", "AdaptiveInstanceNorm", "WScaleLayer",
           "Truncation",
           "model_utils", "get_repulsion_loss", "get_repulsion_loss4", "get_perulsion_loss", "get_uniform_loss_knn", "get_cd_loss", "get_cd_loss2",
           "get_hausdorff_loss", "group_nearest", "get_emd_loss",
           "approxmatch", "MatchCostFunction", "approx_match", "match_cost", "match_cost_dense", "emd_approx_match",
           "augment", "BatchAugment"]
