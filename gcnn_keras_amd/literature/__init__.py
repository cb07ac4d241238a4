from . import INorp  # noqa: F401
