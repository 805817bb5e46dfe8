"""Prediction with trained models: the fold ensemble of the reference's `entry/fugc2025/predict.py` on the GPU, and tiled
prediction with Gaussian blending and mirroring at the images' own resolution; connected-component clean-up of the label maps."""
from .components import compact_ids, connected_components, filter_components, keep_largest_component  # noqa: F401
from .predictor import (EnsemblePredictor, ensemble_predict, ensemble_predict_regions, regions_to_labels,  # noqa: F401
                        sigmoid_accum, sliding_window_predict, softmax_accum, window_accum, window_finalize, window_starts,
                        window_weights)
