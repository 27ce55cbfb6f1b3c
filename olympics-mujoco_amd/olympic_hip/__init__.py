"""olympic_hip: MI355X-native hot path of the olympics-mujoco locomotion environments.

Nothing here imports the CPU oracle; the HIP library is loaded lazily by olympic_hip._ffi and
its absence is an error, not a fallback."""
from . import _abi, specs  # noqa: F401

__all__ = ["_abi", "specs", "DeviceBehavioralCloning", "DeviceSquashedGaussianPolicy", "DeviceSoftQCritic",
           "DeviceReplayMemory", "DeviceIQLearn", "DeviceSQIL", "DeviceLSIQ", "DeviceLSIQH", "DeviceLSIQHC", "DeviceIQSAC",
           "DeviceSQILSAC", "DeviceLSIQSAC", "DeviceLSIQHSAC", "DeviceLSIQHCSAC", "DeviceGaussianInvActionModel",
           "DeviceIQfOSAC", "DeviceLSIQfOSAC", "DeviceLSIQfOHSAC", "DeviceLSIQfOHCSAC", "DeviceLSIQOffline"]


def __getattr__(name):
    # behavioural cloning (bc.py, K24); resolved on first use so that importing the package stays free of torch
    if name in ("DeviceBehavioralCloning", "DeviceSquashedGaussianPolicy"):
        from . import bc
        return getattr(bc, name)
    # the SAC family (iq.py: the critic side K26, the whole agents with the policy side K27)
    if name in ("DeviceSoftQCritic", "DeviceReplayMemory", "DeviceIQLearn", "DeviceSQIL", "DeviceLSIQ", "DeviceLSIQH",
                "DeviceLSIQHC", "DeviceIQSAC", "DeviceSQILSAC", "DeviceLSIQSAC", "DeviceLSIQHSAC", "DeviceLSIQHCSAC"):
        from . import iq
        return getattr(iq, name)
    # the inverse action model of the learning-from-observations agents (iqfo.py, K28)
    if name in ("DeviceGaussianInvActionModel", "DeviceIQfOSAC", "DeviceLSIQfOSAC", "DeviceLSIQfOHSAC", "DeviceLSIQfOHCSAC"):
        from . import iqfo
        return getattr(iqfo, name)
    # offline LS-IQ (iq_offline.py: K26's v0 pass on all-expert batches)
    if name == "DeviceLSIQOffline":
        from . import iq_offline
        return iq_offline.DeviceLSIQOffline
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
