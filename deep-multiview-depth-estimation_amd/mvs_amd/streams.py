"""Extra HIP streams of the inference step: side streams for independent branches of one forward and
one stream per lane of MVSNet's sample-pipelined eval forward.  Callers reach the functions through
the module (``streams._side_stream(...)``), so patching the attribute here reaches every caller."""
import torch

_SIDE_STREAMS = {}
# the lane of MVSNet's sample-pipelined eval forward that is issuing kernels (0: none): every lane gets
# its own side streams, so two lanes' branches never serialise on one stream
_LANE = [0]


def _side_stream(device, which=0, priority=0):
    """Extra HIP streams per device (and pipeline lane) for independent branches of the inference step."""
    key = (torch.device(device).index, which, _LANE[0], priority)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device, priority=priority)
    return _SIDE_STREAMS[key]


def _lane_stream(device, lane):
    """The stream of pipeline lane ``lane`` (MVSNet._forward_pipelined)."""
    key = (torch.device(device).index, "lane", lane)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device)
    return _SIDE_STREAMS[key]
