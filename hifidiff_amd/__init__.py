"""hifidiff_amd: MI355X-native refiner sampling path of HifiDiff."""


def __getattr__(name):
    # `hifidiff_amd.photo` (photo ingest and paste-back) without paying for torch and the library on a bare `import hifidiff_amd`
    if name == "photo":
        import importlib
        return importlib.import_module(".photo", __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
