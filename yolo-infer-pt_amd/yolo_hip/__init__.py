"""MI355X (gfx950) HIP runtime of the YOLOv11 inference path.

`Engine` wraps one yh_handle (include/yolo_hip.h); `nms` is the on-device
non_max_suppression; `Evaluator` (yolo_hip.evaluate) is the batched mAP
evaluation over those detections; `Detector` (yolo_hip.detect) returns detections in
source-image pixels, optionally from tiled inference (`tiles`, `tile_transform`, `merge`),
from BGR or `NV12` video frames on a square or rectangular canvas (`letterbox_frames`,
`rect_canvas`; yolo_hip.preprocess), and `crop_rois` cuts one fixed-size crop per detection from
those frames for a second-stage model (`Crops`);
`Tracker` (yolo_hip.track) gives the detections of video streams identities across frames
(`track`, `track_state`, `Tracks`), with re-identification by appearance when it is given
embeddings (`track_reid`, `embed_quantize`, `embed_similarity`), and with an optimal assignment in
place of the greedy association on request (`assign="optimal"`; `assign` is the batched solver alone), and
with camera-motion compensation (`MotionEstimator`, yolo_hip.motion: the translation between consecutive
frames from their luma; `warp` / `Tracker.update(motion=...)` moves the tracks by it); `Classifier` (yolo_hip.classify) runs a YOLO11-cls second stage on
those crops (`Classified`: class, confidence and embedding per detection); `Gallery` (yolo_hip.gallery)
turns those embeddings into identities across streams and time (`gallery_search`, `gallery_enrol`,
`gallery_workspace`: the k best rows of a large int8 gallery per query on the int8 MFMA). The drop-in module API lives in `nets.nn` / `utils.util`.
"""
from .variants import VARIANTS, Variant, lookup  # noqa: F401


def __getattr__(name):
    # torch-dependent pieces load lazily so `import yolo_hip` stays cheap
    if name in ("Engine", "nms"):
        from . import engine
        return getattr(engine, name)
    if name == "Evaluator":
        from . import evaluate
        return evaluate.Evaluator
    if name in ("Detector", "Detections", "merge"):
        from . import detect
        return getattr(detect, name)
    if name in ("tiles", "tile_transform"):
        from . import detect
        return getattr(detect, name)
    if name in ("NV12", "letterbox_frames", "rect_canvas", "crop_rois", "Crops"):
        from . import preprocess
        return getattr(preprocess, name)
    if name in ("Classifier", "Classified"):
        from . import classify
        return getattr(classify, name)
    if name in ("MotionEstimator", "Motion", "motion_state"):
        from . import motion
        return getattr(motion, name)
    if name in ("Tracker", "Tracks", "track", "track_state", "track_reid", "embed_quantize", "embed_similarity",
                "assign", "warp"):
        # the function shares its name with its module, and importing the module binds the name
        # here: the module is callable as the function (yolo_hip/track.py, at its end)
        import importlib
        mod = importlib.import_module(".track", __name__)
        return mod if name == "track" else getattr(mod, name)
    if name in ("Gallery", "gallery_search", "gallery_enrol", "gallery_workspace"):
        from . import gallery
        return getattr(gallery, name)
    raise AttributeError(name)
