"""CPU: which BLSTM kernel each half layer runs (ops.lstm_fwd_kernel / ops.lstm_bwd_kernel) and which optional weight layouts the model
packs for it (ops.lstm_layouts), pinned in literal tables.  The expected values are the choices of the dispatch chains the planners replaced,
checked against them on the full cross product of shapes, paths, dtypes, reservations and switches.  The plan queries need no GPU: the library
assumes 256 CUs, and so does ops.device_cus here."""
import pytest
import torch

# model: (N, H, K bands, T frames).  SE: the C2 configuration; Flow: C4.
SHAPES = {"SE": (196, 392, 34, 401), "Flow": (384, 768, 48, 501)}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

# (model, path, dtype, B, bf16_copy, reservation, (switch, value), forward kernel, BPTT kernel)
DECISIONS = [
    ('SE', 't', 'bf16', 1, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 4, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 7, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 8, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 14, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 16, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 21, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 33, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 34, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, None, 'clusterx', 'nsplit'),
    ('Flow', 't', 'bf16', 1, False, None, None, 'cluster2', 'split'),
    ('Flow', 't', 'bf16', 2, False, None, None, 'cluster2', 'split'),
    ('Flow', 't', 'bf16', 4, False, None, None, 'cluster2', 'split'),
    ('SE', 'f', 'bf16', 1, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 4, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 7, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 8, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 14, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 16, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 21, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 33, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 34, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 48, False, None, None, 'clusterx', 'stream'),
    ('Flow', 'f', 'bf16', 1, False, None, None, 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, None, 'cluster2', 'stream'),
    ('Flow', 'f', 'bf16', 4, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f16', 1, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 4, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 7, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 8, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 14, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 16, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 21, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 33, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 34, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, None, 'clusterx', 'nsplit'),
    ('Flow', 't', 'f16', 1, False, None, None, 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, None, 'cluster2', 'split'),
    ('Flow', 't', 'f16', 4, False, None, None, 'cluster2', 'split'),
    ('SE', 'f', 'f16', 1, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 4, False, None, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 7, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 8, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 14, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 16, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 21, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 33, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 34, False, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 48, False, None, None, 'clusterx', 'stream'),
    ('Flow', 'f', 'f16', 1, False, None, None, 'cluster2', 'split'),
    ('Flow', 'f', 'f16', 2, False, None, None, 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 4, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 1, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 4, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 7, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 8, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 14, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 16, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 21, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 32, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 33, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 34, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f32', 48, False, None, None, 'stream', 'stream'),
    ('Flow', 't', 'f32', 1, False, None, None, 'stream', 'stream'),
    ('Flow', 't', 'f32', 2, False, None, None, 'stream', 'stream'),
    ('Flow', 't', 'f32', 4, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 1, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 4, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 7, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 8, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 14, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 16, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 21, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 32, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 33, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 34, False, None, None, 'stream', 'stream'),
    ('SE', 'f', 'f32', 48, False, None, None, 'stream', 'stream'),
    ('Flow', 'f', 'f32', 1, False, None, None, 'stream', 'stream'),
    ('Flow', 'f', 'f32', 2, False, None, None, 'stream', 'stream'),
    ('Flow', 'f', 'f32', 4, False, None, None, 'stream', 'stream'),
    ('SE', 't', 'f16', 1, True, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 8, True, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, True, None, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, True, None, None, 'clusterx', 'nsplit'),
    ('Flow', 't', 'f16', 2, True, None, None, 'stream', 'split'),  # bf16_copy: cluster2 cannot write the bf16 copy of h
    ('SE', 'f', 'f16', 1, True, None, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, True, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, True, None, None, 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 48, True, None, None, 'clusterx', 'stream'),
    ('Flow', 'f', 'f16', 2, True, None, None, 'stream', 'stream'),  # bf16_copy: cluster2 cannot write the bf16 copy of h
    ('SE', 't', 'bf16', 4, False, {'co_resident': 84}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, {'co_resident': 84}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 33, False, {'co_resident': 84}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, {'co_resident': 84}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 4, False, {'co_resident': 84}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, {'co_resident': 84}, None, 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, {'co_resident': 84}, None, 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 1, False, {'co_resident': 84}, None, 'cluster2', 'stream'),  # the reservation refuses a cooperative plan that fits without it
    ('SE', 't', 'bf16', 4, False, {'co_resident': 98}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, {'co_resident': 98}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 33, False, {'co_resident': 98}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, {'co_resident': 98}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 4, False, {'co_resident': 98}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, {'co_resident': 98}, None, 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, {'co_resident': 98}, None, 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 1, False, {'co_resident': 98}, None, 'cluster2', 'stream'),  # the reservation refuses a cooperative plan that fits without it
    ('SE', 't', 'bf16', 4, False, {'co_resident': 112}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, {'co_resident': 112}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 33, False, {'co_resident': 112}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, {'co_resident': 112}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 4, False, {'co_resident': 112}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, {'co_resident': 112}, None, 'stream', 'stream'),  # the reservation refuses a cooperative plan that fits without it
    ('Flow', 't', 'bf16', 2, False, {'co_resident': 112}, None, 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 1, False, {'co_resident': 112}, None, 'cluster2', 'stream'),  # the reservation refuses a cooperative plan that fits without it
    ('SE', 't', 'bf16', 4, False, {'prefetch': 8}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, {'prefetch': 8}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 33, False, {'prefetch': 8}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, {'prefetch': 8}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 4, False, {'prefetch': 8}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, {'prefetch': 8}, None, 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, {'prefetch': 8}, None, 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 1, False, {'prefetch': 8}, None, 'cluster2', 'split'),
    ('SE', 't', 'bf16', 4, False, {'comm': 32}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, {'comm': 32}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 33, False, {'comm': 32}, None, 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, {'comm': 32}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 4, False, {'comm': 32}, None, 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, {'comm': 32}, None, 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, {'comm': 32}, None, 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 1, False, {'comm': 32}, None, 'cluster2', 'split'),
    ('SE', 't', 'bf16', 32, False, None, ('SHARED_GPU_RANKS', 2), 'stream', 'stream'),  # no cooperative plan on a shared GPU
    ('SE', 'f', 'bf16', 32, False, None, ('SHARED_GPU_RANKS', 2), 'rwx', 'stream'),  # no cooperative plan on a shared GPU
    ('SE', 't', 'f16', 32, False, None, ('SHARED_GPU_RANKS', 2), 'stream', 'stream'),  # no cooperative plan on a shared GPU
    ('SE', 'f', 'f16', 32, False, None, ('SHARED_GPU_RANKS', 2), 'rwx', 'stream'),  # no cooperative plan on a shared GPU
    ('Flow', 't', 'bf16', 2, False, None, ('SHARED_GPU_RANKS', 2), 'stream', 'stream'),  # no cooperative plan on a shared GPU
    ('SE', 't', 'bf16', 4, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_CLUSTER_LSTM', False), 'rwx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_CLUSTER_LSTM', False), 'rwx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_CLUSTER_LSTM', False), 'stream', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'cluster'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'cluster'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'cluster'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_CLUSTER_LSTM_BWD', True), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_CLUSTERX_LSTM', False), 'stream', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_CLUSTERX_LSTM', False), 'stream', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_CLUSTERX_LSTM', False), 'rwx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('USE_CLUSTERX_LSTM', False), 'stream', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_CLUSTERX_LSTM', False), 'stream', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_CLUSTERX_LSTM', False), 'rwx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_CLUSTERX_LSTM', False), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('BAND_CLUSTERX', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('BAND_CLUSTERX', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('BAND_CLUSTERX', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('BAND_CLUSTERX', False), 'cluster', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('BAND_CLUSTERX', False), 'stream', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('BAND_CLUSTERX', False), 'rwx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('BAND_CLUSTERX', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('BAND_CLUSTERX', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('BAND_CLUSTERX', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('BAND_CLUSTERX', False), 'cluster', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('BAND_CLUSTERX', False), 'stream', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('BAND_CLUSTERX', False), 'rwx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('BAND_CLUSTERX', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('BAND_CLUSTERX', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('BAND_CLUSTERX', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('BAND_CLUSTERX', False), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'stream', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'stream', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('TIME_CLUSTERX_ROUNDS', False), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('CLUSTER2_H', ()), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('CLUSTER2_H', ()), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('CLUSTER2_H', ()), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('CLUSTER2_H', ()), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('CLUSTER2_H', ()), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('CLUSTER2_H', ()), 'stream', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('CLUSTER2_H', ()), 'stream', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('CLUSTER2_H', ()), 'stream', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('CLUSTER2_H', ()), 'stream', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_WIDE_LSTM', False), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_WIDE_LSTM', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_WIDE_LSTM', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_WIDE_LSTM', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_WIDE_LSTM', False), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_RW_LSTM', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_RW_LSTM', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_RW_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_RW_LSTM', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_RW_LSTM', False), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_RW_LSTM', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_RW_LSTM', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_RW_LSTM', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_RW_LSTM', False), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_RWX_LSTM', False), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_RWX_LSTM', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_RWX_LSTM', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_RWX_LSTM', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_RWX_LSTM', False), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('BAND_PATH_NO_CLUSTER', True), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 32, False, None, ('BAND_PATH_NO_CLUSTER', True), 'clusterx', 'nsplit'),
    ('SE', 't', 'bf16', 48, False, None, ('BAND_PATH_NO_CLUSTER', True), 'clusterx', 'nsplit'),
    ('SE', 'f', 'bf16', 1, False, None, ('BAND_PATH_NO_CLUSTER', True), 'stream', 'nsplit'),
    ('SE', 'f', 'bf16', 8, False, None, ('BAND_PATH_NO_CLUSTER', True), 'stream', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('BAND_PATH_NO_CLUSTER', True), 'rwx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('BAND_PATH_NO_CLUSTER', True), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 32, False, None, ('BAND_PATH_NO_CLUSTER', True), 'clusterx', 'nsplit'),
    ('SE', 't', 'f16', 48, False, None, ('BAND_PATH_NO_CLUSTER', True), 'clusterx', 'nsplit'),
    ('SE', 'f', 'f16', 1, False, None, ('BAND_PATH_NO_CLUSTER', True), 'stream', 'nsplit'),
    ('SE', 'f', 'f16', 8, False, None, ('BAND_PATH_NO_CLUSTER', True), 'stream', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('BAND_PATH_NO_CLUSTER', True), 'rwx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('BAND_PATH_NO_CLUSTER', True), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('BAND_PATH_NO_CLUSTER', True), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('BAND_PATH_NO_CLUSTER', True), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('BAND_PATH_NO_CLUSTER', True), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 't', 'f16', 32, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 't', 'f16', 48, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'split'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_SPLIT_LSTM_BWD', True), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_SPLIT_LSTM_BWD', True), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_SPLIT_LSTM_BWD', True), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_SPLIT_LSTM_BWD', True), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_SPLIT_LSTM_BWD', True), 'cluster2', 'stream'),
    ('SE', 't', 'bf16', 4, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 't', 'bf16', 32, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 't', 'bf16', 48, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 1, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 8, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 'f', 'bf16', 32, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 4, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 32, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 't', 'f16', 48, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 1, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 8, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('SE', 'f', 'f16', 32, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'clusterx', 'stream'),
    ('Flow', 't', 'bf16', 2, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'cluster2', 'split'),
    ('Flow', 't', 'f16', 2, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'cluster2', 'split'),
    ('Flow', 'f', 'bf16', 2, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'cluster2', 'stream'),
    ('Flow', 'f', 'f16', 2, False, None, ('USE_NSPLIT_LSTM_BWD', False), 'cluster2', 'stream'),
]

# (model, path, dtype, (switch, value), optional layouts packed for the half layer)
LAYOUTS = [
    ('SE', 't', 'bf16', None, 'whhb whhq wihq'),  # H = 392: the time path has no wx
    ('SE', 'f', 'bf16', None, 'whhb whhq wihq wx'),
    ('SE', 't', 'f16', None, 'whhq wihq'),  # H = 392: the time path has no wx
    ('SE', 'f', 'f16', None, 'whhq wihq wx'),
    ('SE', 't', 'f32', None, ''),  # H = 392: the time path has no wx
    ('SE', 'f', 'f32', None, ''),
    ('Flow', 't', 'bf16', None, 'whhq'),  # H = 768: no clusterx / rwx / wide kernel
    ('Flow', 'f', 'bf16', None, 'whhq'),  # H = 768: no clusterx / rwx / wide kernel
    ('Flow', 't', 'f16', None, 'whhq'),  # H = 768: no clusterx / rwx / wide kernel
    ('Flow', 'f', 'f16', None, 'whhq'),  # H = 768: no clusterx / rwx / wide kernel
    ('Flow', 't', 'f32', None, ''),
    ('Flow', 'f', 'f32', None, ''),
    ('SE', 't', 'bf16', ('USE_CLUSTER_LSTM', False), 'whhb'),
    ('SE', 'f', 'bf16', ('USE_CLUSTER_LSTM', False), 'whhb wx'),
    ('SE', 't', 'f16', ('USE_CLUSTER_LSTM', False), ''),
    ('SE', 'f', 'f16', ('USE_CLUSTER_LSTM', False), 'wx'),
    ('Flow', 't', 'bf16', ('USE_CLUSTER_LSTM', False), ''),
    ('Flow', 'f', 'bf16', ('USE_CLUSTER_LSTM', False), ''),
    ('Flow', 't', 'f16', ('USE_CLUSTER_LSTM', False), ''),
    ('Flow', 'f', 'f16', ('USE_CLUSTER_LSTM', False), ''),
    ('SE', 't', 'bf16', ('USE_CLUSTER_LSTM_BWD', True), 'whhTq whhb whhq wihq'),
    ('SE', 'f', 'bf16', ('USE_CLUSTER_LSTM_BWD', True), 'whhTq whhb whhq wihq wx'),
    ('Flow', 't', 'bf16', ('USE_CLUSTER_LSTM_BWD', True), 'whhTq whhq'),
    ('Flow', 'f', 'bf16', ('USE_CLUSTER_LSTM_BWD', True), 'whhTq whhq'),
    ('SE', 't', 'bf16', ('USE_CLUSTERX_LSTM', False), 'whhb whhq'),
    ('SE', 'f', 'bf16', ('USE_CLUSTERX_LSTM', False), 'whhb whhq wx'),
    ('SE', 't', 'f16', ('USE_CLUSTERX_LSTM', False), 'whhq'),
    ('SE', 'f', 'f16', ('USE_CLUSTERX_LSTM', False), 'whhq wx'),
    ('SE', 'f', 'bf16', ('BAND_CLUSTERX', False), 'whhb whhq wx'),  # H = 392: the band path reads wihq only in rounds
    ('SE', 'f', 'f16', ('BAND_CLUSTERX', False), 'whhq wx'),  # H = 392: the band path reads wihq only in rounds
    ('SE', 'f', 'bf16', ('USE_RW_LSTM', False), 'whhb whhq wihq'),
    ('SE', 'f', 'f16', ('USE_RW_LSTM', False), 'whhq wihq'),
    ('SE', 'f', 'bf16', ('USE_RWX_LSTM', False), 'whhb whhq wihq'),
    ('SE', 'f', 'f16', ('USE_RWX_LSTM', False), 'whhq wihq'),
    ('SE', 'f', 'bf16', ('BAND_PATH_NO_CLUSTER', True), 'whhb wx'),  # no band-path kernel reads whhq / wihq then
    ('SE', 'f', 'f16', ('BAND_PATH_NO_CLUSTER', True), 'wx'),  # no band-path kernel reads whhq / wihq then
]


def _dims(model, dtype):
    from urgent2026_challenge_track1_amd import ops
    N, H, K, T = SHAPES[model]
    return N, H, K, T, ops.kpad(N, dtype), ops.kpad(ops.pad_to(H, 16), dtype)


def _seqmap(path, B, T, K):
    if path == "t":
        return dict(n_seq=B * K, seq_len=T, inner=K, outer=T * K, stride=K)
    return dict(n_seq=B * T, seq_len=K, inner=1, outer=K, stride=1)


@pytest.fixture
def ops(lib, monkeypatch):
    from urgent2026_challenge_track1_amd import ops
    monkeypatch.setattr(ops, "device_cus", lambda: 256)
    return ops


@pytest.mark.parametrize("model,path,dtype,B,bf16_copy,res,switch,fwd,bwd", DECISIONS)
def test_kernel_choice(ops, monkeypatch, model, path, dtype, B, bf16_copy, res, switch, fwd, bwd):
    if switch:
        monkeypatch.setattr(ops, *switch)
    dt = DTYPES[dtype]
    N, H, K, T, Np, Hp = _dims(model, dt)
    sm = _seqmap(path, B, T, K)
    with ops.reserve_cus(**(res or {})):
        got = (ops.lstm_fwd_kernel(H, Hp, N, Np, dt, path, sm, bf16_copy), ops.lstm_bwd_kernel(H, Hp, N, Np, dt, path, sm))
    assert got == (fwd, bwd)


@pytest.mark.parametrize("model,path,dtype,switch,layouts", LAYOUTS)
def test_packed_layouts(ops, monkeypatch, model, path, dtype, switch, layouts):
    if switch:
        monkeypatch.setattr(ops, *switch)
    dt = DTYPES[dtype]
    N, H, K, T, Np, Hp = _dims(model, dt)
    lay = ops.lstm_layouts(H, Hp, N, Np, dt, path)
    assert lay == set(layouts.split())


def test_a_refused_plan_counts_once(ops):
    """C2 time path beside the 84 workgroups of the second queue: the cluster plan is refused (the kernel then runs in rounds), once."""
    N, H, K, T, Np, Hp = _dims("SE", torch.bfloat16)
    with ops.reserve_cus(co_resident=84):
        before = ops.COOP_REFUSALS
        assert ops.lstm_fwd_kernel(H, Hp, N, Np, torch.bfloat16, "t", _seqmap("t", 32, T, K)) == "clusterx"
        assert ops.COOP_REFUSALS - before == 1
