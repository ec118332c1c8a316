"""ta3n_amd: MI355X-native (gfx950) implementation of TA3N's temporal-adversarial
train step behind the reference's VideoModel.forward()/opts.py surface.

Importing the package never loads the HIP library; the first compute call does,
and raises if it is missing (there is no CPU fallback).
"""
__version__ = "0.1.0"


def __getattr__(name):      # Scorer on first use: importing the package stays free of torch and of the HIP library
    if name == "Scorer":
        from .scoring import Scorer
        return Scorer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
