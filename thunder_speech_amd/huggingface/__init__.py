"""transformers checkpoints on the HIP path: CTC modules (compatibility.py) and audio classification heads (classification.py).  The names
below are resolved on first use, so importing a submodule of this package loads nothing else."""

__all__ = ["AudioClassifierModule", "classifier_from_huggingface", "load_huggingface_classifier"]


def __getattr__(name):
    if name in __all__:
        from . import classification
        return getattr(classification, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
