"""pnpp_hip -- Python host side of the MI355X-native PointNet++ / von-Mises-KL training path.

    _lib    ctypes binding of libpnpp_hip.so (C ABI in include/pnpp_hip.h); no fallback
    ops     argument checking, workspaces, torch.autograd glue
    build   hipcc build of the shared library (gfx950)
    optim   flat-buffer Adam / gradient clipping on the device
    dist    one-process-per-GPU data parallelism (RCCL all-reduce of one flat gradient buffer)
    inference  Predictor: forward-only evaluation, one fused launch per set-abstraction level
    augment Augment: a fresh yaw per cloud and draw on the device, orientation targets moved along
    decode  decode / AngularErrors: von-Mises parameters to orientations, orientations to angular-error statistics, on the device
    normals estimate_normals / with_normals: surface normals of xyz-only clouds (fused kNN + PCA), on the device
    symmetry yaw_profile / yaw_symmetry / symmetric_targets: a cloud's yaw symmetry from its self-Chamfer profile, on the device
"""
__all__ = ["ops", "build", "optim", "dist", "sampling", "inference", "augment", "decode", "normals", "symmetry", "Predictor"]


def __getattr__(name):
    if name == "Predictor":   # resolved on first use: importing the package stays free of torch
        from .inference import Predictor
        return Predictor
    raise AttributeError(f"module 'pnpp_hip' has no attribute '{name}'")
