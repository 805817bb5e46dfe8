"""Prediction with trained models: the fold ensemble of the reference's `entry/fugc2025/predict.py` on the GPU."""
from .predictor import EnsemblePredictor, ensemble_predict, softmax_accum  # noqa: F401
