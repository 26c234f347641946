from .logit_lens import VAELogitLens  # noqa: F401
