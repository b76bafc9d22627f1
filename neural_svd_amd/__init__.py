"""neural_svd_amd: MI355X-native NestedLoRA / NeuralSVD PDE training step.

The compute lives in ``libnsvd_hip.so`` (hand-written HIP for gfx950, C ABI in ``include/nsvd.h``);
this package is the host-side mirror of the reference's Python interface for that path.
"""
from . import _lib  # noqa: F401

__all__ = ["_lib", "SketchyRetrieval", "evaluate_truncations", "Nystrom", "run_nystrom", "NystromSVD", "DotKernelOperator",
           "SpIN", "SpinKernelTrainer", "SpINx", "SpinxKernelTrainer", "NefKernelTrainer", "PairedFunctions", "KernelSvdTrainer", "gaussian_cross_singular_values",
           "gaussian_cross_modes", "kernel_singular_values", "DenseCrossOperator", "DenseSvdTrainer"]


def __getattr__(name):
    # the retrieval evaluation (retrieval.py) is exported here; resolved on first use, so that importing the package
    # stays as light as the ctypes binding
    if name in ("SketchyRetrieval", "evaluate_truncations"):
        from . import retrieval
        return getattr(retrieval, name)
    if name in ("Nystrom", "run_nystrom"):  # the Nystrom baseline (nystrom.py), the same way
        from . import nystrom
        return getattr(nystrom, name)
    if name == "NystromSVD":  # the truncated-SVD baseline of the kernel SVD operators (nystrom_svd.py), the same way
        from . import nystrom_svd
        return nystrom_svd.NystromSVD
    if name == "DotKernelOperator":  # the dot-product kernel operator (kernel_ops.py), the same way
        from . import kernel_ops
        return kernel_ops.DotKernelOperator
    if name in ("SpIN", "SpinKernelTrainer"):  # SpIN on the kernel-operator path (spin.py), the same way
        from . import spin
        return getattr(spin, name)
    if name in ("SpINx", "SpinxKernelTrainer"):  # SpINx on the kernel-operator path (spinx.py), the same way
        from . import spinx
        return getattr(spinx, name)
    if name == "NefKernelTrainer":  # NeuralEF on the kernel-operator path (neuralef.py), the same way
        from . import neuralef
        return neuralef.NefKernelTrainer
    if name in ("PairedFunctions", "KernelSvdTrainer", "DenseSvdTrainer"):  # the kernel SVD path (kernel_svd.py), the same way
        from . import kernel_svd
        return getattr(kernel_svd, name)
    if name in ("gaussian_cross_singular_values", "gaussian_cross_modes", "kernel_singular_values",
                "DenseCrossOperator"):
        from . import kernel_ops
        return getattr(kernel_ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
