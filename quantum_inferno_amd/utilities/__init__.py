"""Host-side scalar helpers on the TFR path (mirror of quantum_inferno/utilities)."""
from . import sampling  # noqa: F401,E402
