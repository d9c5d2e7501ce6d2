"""Drop-in for the reference's top-level `utils.helpers` module (reference main.py:12:
`from utils.helpers import compute_similarity, draw_bbox_info, draw_bbox`)."""
from scrfd_arcface_facerecognition_amd.utils.helpers import (  # noqa: F401
    bgr_to_nv12, cluster_embeddings, coast_tracks, compute_similarities, compute_similarity, distance2bbox, distance2kps, draw_bbox, draw_bbox_info, draw_faces, draw_faces_nv12,
    estimate_norm, identity_templates, match_gallery,
    measure_crops, norm_crop_image, nv12_to_bgr, redact_faces, reference_alignment, relink_state, relink_tracks, score_distribution)
