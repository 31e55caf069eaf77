"""insar_unet_ca_amd — MI355X-native U-Net-CA training hot path (drop-in for
Createroner/InSAR-Unet-CA's Unet-ChannalAttention.py model/loss/optimizer entry points)."""
from ._lib import InsarError, LIB_PATH  # noqa: F401
from .data import DevicePrefetcher, ShardedSampler, SyntheticTiles, VOCSegDataset, make_loader, reference_transforms  # noqa: F401
from .loss import CrossEntropyLoss, DiceCELoss, DiceLoss, FocalLoss, class_weights, label_histogram  # noqa: F401
from .modules import ChannelAttentionModule, DoubleConv, MaxPool2d, SELayer, UNet  # noqa: F401
from .deeplab import DeepLabV3_SingleChannel_Attn  # noqa: F401
from .fcn import FCN_SingleChannel, FCN_SingleChannel_SE  # noqa: F401
from .spatial import SpatialAttention, UNet as UNetSpatialAttention  # noqa: F401
from .optim import Adam, AdamW, LRSchedule, split_decay_groups  # noqa: F401
from .graph import GraphedTrainStep  # noqa: F401
from .train import compute_metrics, save_history, train_model, validate_model  # noqa: F401
from .infer import (ScenePredictor, detect_scene, evaluate_scene, gather_tiles, plan_tiles, predict_scene, select_tiles,  # noqa: F401
                    stitch_logits, tile_census, window_1d)
from .regions import label_regions  # noqa: F401
from .score import DetectionScore, match_from_overlaps, match_regions, region_overlaps  # noqa: F401
from .augment import Augment  # noqa: F401
from .distance import DistanceScratch, boundary_counts, boundary_iou, distance_transform, expand_labels, void_band  # noqa: F401
from .crops import CropIndex, SceneCrops, draw_crops, gather_crops  # noqa: F401
from .outlines import OutlineScratch, region_outlines, to_geojson, to_polygons  # noqa: F401
from .simplify import SimplifyScratch, simplify_outlines  # noqa: F401
from .contours import ContourScratch, contour_lines, contour_polygons, contours_to_geojson, lines_to_coords  # noqa: F401
from .contours import ContourSimplifyScratch, simplify_contours  # noqa: F401
from .focal import box_taps, focal_tile, gaussian_taps, gradient_raster, rank_filter, smooth_raster  # noqa: F401
from .skeletons import SkeletonScratch, skeleton_table, thin_regions  # noqa: F401
from .zonal import ZonalScratch, percentile, region_stats  # noqa: F401
from .split import SplitScratch, split_regions  # noqa: F401
from .rasterise import PolygonTable, RasterScratch, from_geojson, labels_from_geojson, pack_polygons, rasterise_polygons  # noqa: F401
from .warp import WarpSpec, draw_warps, gather_warped, grid_matrix, multilook, warp_raster  # noqa: F401
from .stack import DetectionStack, StackScratch, follow_sites, site_series  # noqa: F401
from .sieve import SieveScratch, region_adjacency, sieve_regions  # noqa: F401
from .hysteresis import HysteresisScratch, hysteresis_regions  # noqa: F401
from .reconstruct import ReconstructScratch, fill_sinks, h_dome, reconstruct_raster, reconstruct_tile, regional_extrema  # noqa: F401

__all__ = ["UNet", "DeepLabV3_SingleChannel_Attn", "DoubleConv", "SELayer", "ChannelAttentionModule", "MaxPool2d", "CrossEntropyLoss", "DiceLoss", "DiceCELoss", "Adam", "GraphedTrainStep",
           "compute_metrics", "train_model", "validate_model", "save_history", "VOCSegDataset", "SyntheticTiles",
           "ShardedSampler", "DevicePrefetcher", "make_loader", "reference_transforms", "InsarError", "LIB_PATH",
           "SpatialAttention", "UNetSpatialAttention", "FCN_SingleChannel", "FCN_SingleChannel_SE",
           "ScenePredictor", "predict_scene", "stitch_logits", "plan_tiles", "window_1d", "gather_tiles", "tile_census", "select_tiles",
           "FocalLoss", "class_weights", "label_histogram", "label_regions", "detect_scene", "Augment",
           "AdamW", "LRSchedule", "split_decay_groups",
           "region_overlaps", "match_regions", "match_from_overlaps", "DetectionScore", "evaluate_scene",
           "DistanceScratch", "distance_transform", "void_band", "expand_labels", "boundary_counts", "boundary_iou",
           "CropIndex", "SceneCrops", "draw_crops", "gather_crops",
           "OutlineScratch", "region_outlines", "to_polygons", "to_geojson", "SimplifyScratch", "simplify_outlines",
           "ContourScratch", "contour_lines", "contour_polygons", "contours_to_geojson", "lines_to_coords",
           "ContourSimplifyScratch", "simplify_contours",
           "smooth_raster", "rank_filter", "gradient_raster", "box_taps", "gaussian_taps", "focal_tile",
           "SkeletonScratch", "thin_regions", "skeleton_table",
           "PolygonTable", "RasterScratch", "pack_polygons", "from_geojson", "rasterise_polygons", "labels_from_geojson",
           "ZonalScratch", "region_stats", "percentile", "SplitScratch", "split_regions",
           "warp_raster", "grid_matrix", "multilook", "WarpSpec", "draw_warps", "gather_warped",
           "DetectionStack", "StackScratch", "site_series", "follow_sites",
           "SieveScratch", "region_adjacency", "sieve_regions"]
__all__ += ["HysteresisScratch", "hysteresis_regions"]
__all__ += ["ReconstructScratch", "reconstruct_raster", "fill_sinks", "h_dome", "regional_extrema", "reconstruct_tile"]
