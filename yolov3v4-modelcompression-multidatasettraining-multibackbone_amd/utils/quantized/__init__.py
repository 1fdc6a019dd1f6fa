"""Quantisation modules.

``quantized_ptq_cos`` (the post-training path the int8 HIP engine lowers), ``quantized_google``
(BN-folding quantization-aware training, ``--quantized 1``, its quantisers on the fused kernels of ``engine/qat.py``) and
``quantized_TPSQ`` (learnable power-of-two scales, ``--quantized 2``, on the fused kernels of ``engine/tpsq.py``) are implemented in
this package and need no checkout of the reference.  The reference's other research quantisers are not: when a checkout of the
reference is present they resolve to its unmodified files (this package's directory comes first on the search path, so a module that
exists here always wins), and where none is present importing them raises ``ModuleNotFoundError``.
"""
import os as _os

_ref = _os.path.join(_os.environ.get('YOLO_REFERENCE_ROOT', '/root/reference'), 'utils', 'quantized')
if _os.path.isdir(_ref) and _ref not in __path__:
    __path__.append(_ref)
