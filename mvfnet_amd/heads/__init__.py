from .tsn_clshead import TSNClsHead, class_balanced_weights

__all__ = ["TSNClsHead", "class_balanced_weights"]
