"""Stand-ins for the reference's native extensions under the module names the reference imports.

    import spgan.compat
    spgan.compat.install()
    from metrics.pointops import pointops            # Generation/modules.py:17       -> spgan.pointops
    from pointops import pointops_util               # Common/loss_utils.py:13        -> spgan.pointops
    from CD_EMD.emd_ import emd_module               # Common/loss_utils.py:20        -> spgan.metrics (emdModule, emdFunction)
    from CD_EMD.cd.chamferdist import ChamferDistance as CD                           # -> spgan.metrics.ChamferDistance
    from pointnet2.pointnet2_modules import PointnetSAModule, PointnetSAModuleMSG     # model.py / Generator.py / modules.py (commented there)
    from metrics.pointnet2 import pointnet2_utils, pytorch_utils                      # -> spgan.pointnet2_utils, spgan.pytorch_utils
    from StructuralLosses.match_cost import match_cost                                # metrics/evaluation_metrics.py:9 -> spgan.approxmatch
    from metrics.StructuralLosses.nn_distance import nn_distance                      # metrics/evaluation_metrics.py:10 -> spgan.metrics

`install()` puts lightweight module objects into sys.modules; each forwards attribute look-ups to the spgan module behind it, so the names
resolve to the very objects of this package.  A name that already resolves to a real module (one in sys.modules, or one the import system
can find) is left alone unless force=True; parent packages (`metrics`, `CD_EMD`, ...) are registered only where none is importable, also
under force.  `uninstall()` puts sys.modules back as `install()` found it.  Neither call touches the GPU or loads the shared library.
"""
from __future__ import annotations

import importlib
import importlib.util
import sys
import types
from typing import Dict, List, Optional

# name -> the spgan module behind it (None: a bare parent package)
STAND_INS: Dict[str, Optional[str]] = {
    "metrics": None,
    "metrics.pointops": "spgan.pointops",
    "metrics.pointops.pointops": "spgan.pointops",
    "metrics.pointops.pointops_util": "spgan.pointops",
    "pointops": "spgan.pointops",
    "pointops.pointops_util": "spgan.pointops",
    "CD_EMD": None,
    "CD_EMD.emd_": None,
    "CD_EMD.emd_.emd_module": "spgan.metrics",
    "metrics.emd": None,
    "metrics.emd.emd_module": "spgan.metrics",
    "emd_module": "spgan.metrics",
    "CD_EMD.cd": None,
    "CD_EMD.cd.chamferdist": "spgan.metrics",
    "CD_EMD.cd.chamferdist.ChamferDistance": "spgan.metrics",
    "expansion_penalty_module": "spgan.expansion_penalty",
    "MDS_module": "spgan.mds",
    "pointnet2": None,
    "pointnet2.pointnet2_utils": "spgan.pointnet2_utils",
    "pointnet2.pointnet2_modules": "spgan.pointnet2_modules",
    "pointnet2.pytorch_utils": "spgan.pytorch_utils",
    "metrics.pointnet2": None,
    "metrics.pointnet2.pointnet2_utils": "spgan.pointnet2_utils",
    "metrics.pointnet2.pointnet2_modules": "spgan.pointnet2_modules",
    "metrics.pointnet2.pytorch_utils": "spgan.pytorch_utils",
    "metrics.pointnet2_ops": None,
    "metrics.pointnet2_ops.pointnet2_utils": "spgan.pointnet2_utils",
    "metrics.pointnet2_ops.pointnet2_modules": "spgan.pointnet2_modules",
    "metrics.pointnet2_ops.pytorch_utils": "spgan.pytorch_utils",
    "metrics.pointnet2_utils": "spgan.pointnet2_utils",
    "StructuralLosses": None,
    "StructuralLosses.match_cost": "spgan.approxmatch",
    "StructuralLosses.nn_distance": "spgan.metrics",
    "metrics.StructuralLosses": None,
    "metrics.StructuralLosses.match_cost": "spgan.approxmatch",
    "metrics.StructuralLosses.nn_distance": "spgan.metrics",
}
# children that are NOT set as attributes of their parent: `from CD_EMD.cd.chamferdist import ChamferDistance` is the class, as the
# reference's own __init__ arranges
_NO_ATTRIBUTE = {"CD_EMD.cd.chamferdist.ChamferDistance"}

_MARK = "__spgan_compat__"
_installed: Dict[str, Optional[types.ModuleType]] = {}       # name -> what sys.modules held before (None: nothing)
_attributes: List[tuple] = []                                # (parent stub, attribute) set by install


def _ours(mod) -> bool:
    return getattr(mod, _MARK, False) is True


def _resolves(name: str) -> bool:
    """Does `name` already mean a real module?"""
    if name in sys.modules:
        return not _ours(sys.modules[name])
    parent = name.rpartition(".")[0]
    if parent and _ours(sys.modules.get(parent)):
        return False                                         # below one of our stand-ins nothing else can be found
    try:
        return importlib.util.find_spec(name) is not None
    except Exception:                                        # a parent that is no package, or one whose import fails
        return False


def _make(name: str, backing: Optional[str], is_package: bool) -> types.ModuleType:
    mod = types.ModuleType(name, "spgan.compat stand-in for %s%s" % (name, " -> " + backing if backing else ""))
    setattr(mod, _MARK, True)
    if is_package:
        mod.__path__ = []                                    # a package with nothing on disk
    if backing is not None:
        target = importlib.import_module(backing)

        def __getattr__(attr, _target=target, _name=name):
            try:
                return getattr(_target, attr)
            except AttributeError:
                raise AttributeError("module %r (spgan.compat stand-in for %s) has no attribute %r" % (_name, _target.__name__, attr)) from None

        def __dir__(_target=target):
            return sorted(set(dir(_target)))

        mod.__getattr__ = __getattr__
        mod.__dir__ = __dir__
        mod.__wrapped__ = target
    return mod


def install(force: bool = False) -> List[str]:
    """Register the stand-ins; returns the names registered by this call."""
    added = []
    names = sorted(STAND_INS, key=lambda n: (n.count("."), n))            # parents before children
    packages = {n.rpartition(".")[0] for n in names if "." in n}
    for name in names:
        backing = STAND_INS[name]
        if _ours(sys.modules.get(name)):
            continue                                                      # installed already
        replace = force and backing is not None
        if not replace and _resolves(name):
            continue
        previous = sys.modules.get(name)
        mod = _make(name, backing, name in packages)
        sys.modules[name] = mod
        _installed[name] = previous
        added.append(name)
        parent, _, leaf = name.rpartition(".")
        if parent and name not in _NO_ATTRIBUTE and _ours(sys.modules.get(parent)):
            setattr(sys.modules[parent], leaf, mod)
            _attributes.append((sys.modules[parent], leaf))
    return added


def uninstall() -> List[str]:
    """Remove exactly what install() added (a module replaced under force=True comes back); returns the names removed."""
    removed = []
    for parent, leaf in _attributes:
        parent.__dict__.pop(leaf, None)
    del _attributes[:]
    for name in sorted(_installed, key=lambda n: -n.count(".")):
        previous = _installed[name]
        if _ours(sys.modules.get(name)):
            if previous is None:
                del sys.modules[name]
            else:
                sys.modules[name] = previous
            removed.append(name)
    _installed.clear()
    return removed
