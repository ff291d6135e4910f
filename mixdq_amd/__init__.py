__all__ = ["Sampler"]


def __getattr__(name):          # (lazy: `python -m mixdq_amd.build` must run before numpy / torch are needed)
    if name == "Sampler":
        from mixdq_amd.sampler import Sampler
        return Sampler
    raise AttributeError(f"module 'mixdq_amd' has no attribute {name!r}")
