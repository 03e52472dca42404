"""mivp_amd -- MI355X-native (gfx950) Swin-UNETR hot path.

Host side (this package): the reference's ``SwinUnetR(conf)`` nn.Module surface
and the data-parallel training-step harness, in Python on PyTorch-ROCm (device
memory, streams, torch.distributed only).  Device side: hand-written HIP kernels
behind the C ABI of ``include/mivp.h`` (``libmivp_hip.so``, built in-tree by
``build.py``).  No CPU fallback: ops raise if the library is missing or the
tensors are not on the GPU.
"""
from . import _lib, geometry  # noqa: F401

__all__ = ["_lib", "geometry"]


def __getattr__(name):
    # heavy modules are imported lazily so that `import mivp_amd` stays cheap
    if name in ("swin_ops", "ops", "swin_unetr", "train", "multiview", "inference", "surface",
                "components", "scan", "regions", "shape", "augment", "calibration", "scanstats", "window_fit",
                "skeleton", "otsu", "prompting", "transfer", "multilabel", "clicks", "strokes", "geodesic"):
        import importlib
        return importlib.import_module(f"mivp_amd.{name}")
    if name == "SwinUnetR":
        from .swin_unetr import SwinUnetR
        return SwinUnetR
    if name in ("SlidingWindowPredictor", "predict_volume", "evaluate_volume", "evaluate_volume_surface",
                "predict_scan_volume", "evaluate_volume_lesions", "evaluate_volume_calibration", "WindowSkip", "WindowFit",
                "foreground_box", "AutoForeground"):
        from . import inference
        return getattr(inference, name)
    if name in ("surface_map", "distance_transform_sq", "surface_metrics"):
        from . import surface
        return getattr(surface, name)
    if name in ("label_components", "postprocess_labels"):
        from . import components
        return getattr(components, name)
    if name in ("region_stats", "lesion_metrics", "lesion_score_metrics", "RegionTable", "LesionReport", "region_shape",
                "RegionShape"):
        from . import regions
        return getattr(regions, name)
    if name in ("skeletonize", "skeleton_stats", "centerline_metrics", "evaluate_volume_centerline", "SkeletonResult",
                "SkeletonStats", "CenterlineReport"):
        from . import skeleton
        return getattr(skeleton, name)
    if name in ("calibration_tables", "CalibrationReport"):
        from . import calibration
        return getattr(calibration, name)
    if name in ("ScanGeometry", "prepare_scan", "prepare_labels", "restore_labels", "restore_labels_from_logits"):
        from . import scan
        return getattr(scan, name)
    if name in ("scan_histogram", "window_slot", "IntensityWindow", "ScanHistogram", "WindowSlot", "ScanReport", "OtsuSlot",
                "otsu_slot", "foreground_mask", "window_slot_above"):
        from . import scanstats
        return getattr(scanstats, name)
    if name in ("IntensityTransfer", "TransferTable", "LandmarkSlot", "LandmarkBank", "equalize_table", "match_table",
                "scan_landmarks", "landmark_table", "apply_table"):
        from . import transfer
        return getattr(transfer, name)
    if name in ("IntensityDraws", "IntensitySlot", "draw_intensity", "augment_intensity", "FilterDraws", "FilterSlot",
                "draw_filters", "augment_filters"):
        from . import augment
        return getattr(augment, name)
    if name in ("InputPrompt", "PromptedModel", "build_prompt_optimizer", "input_gradient", "saliency_map", "fgsm"):
        from . import prompting
        return getattr(prompting, name)
    if name in ("LabelGroups", "MultiLabelSpec", "MultiLabelLoss", "multilabel_loss", "decode_groups", "group_counts",
                "group_scores", "evaluate_volume_groups"):
        from . import multilabel
        return getattr(multilabel, name)
    if name in ("ClickSlot", "GuidedModel", "encode_clicks", "simulate_clicks", "simulate_clicks_from_logits",
                "simulate_clicks_ws", "click_rounds", "refine_volume"):
        from . import clicks
        return getattr(clicks, name)
    if name in ("StrokeSlot", "StrokeModel", "encode_strokes", "simulate_box", "simulate_scribbles", "strokes_ws",
                "draw_box_jitter", "scribble_rounds", "box_then_scribbles"):
        from . import strokes
        return getattr(strokes, name)
    if name in ("GeodesicField", "GeodesicModel", "geodesic_ws", "seed_mask", "geodesic_distance", "encode_geodesic",
                "geodesic_rounds"):
        from . import geodesic
        return getattr(geodesic, name)
    raise AttributeError(name)
