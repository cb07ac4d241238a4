"""Label scalers on the engine (kgcnn/data/transform/scaler): the extensive energy / force scalers."""
from .mol import ExtensiveMolecularLabelScaler  # noqa: F401
from .force import EnergyForceExtensiveLabelScaler  # noqa: F401
