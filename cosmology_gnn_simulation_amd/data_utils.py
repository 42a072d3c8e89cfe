"""Drop-in for the reference's ``data_utils`` module: window -> graph.

``preprocess`` keeps the reference signature and returns a ``Data`` with the same
attributes (reference data_utils.py:72-228) but builds the periodic k-NN graph and
its edge features on the GPU (``cgnn_knn_periodic``) instead of running
``torch_cluster.knn`` over a 27x ghost-extended copy on one CPU thread
(:148-164), and the node features in one kernel.  Only the training targets
(:166-214, used by ``train.py`` alone) stay torch element-wise expressions.

Faithfulness notes
* random-walk noise is drawn on the CPU with the reference's exact call sequence
  (``randn_like`` on ``[N, W-1, 3]`` then ``[N, W-1, 1]``, even when
  ``noise_std == 0``, :47,:63), so seeded runs see the same noise and the same RNG
  stream afterwards;
  ``noise_rng="device"`` (extension) instead makes the noise, the features and the targets in one kernel
  (``cgnn_training_sample``) from a counter-based generator: the reference's distribution and arithmetic, not its stream;
* node features (wrap, velocities, normalisation: :91-145) come from one HIP kernel
  (``cgnn_window_features``) with the reference's float32 operation order;
* edge displacements use the un-shifted sender (not minimum-image), as :151-164 do;
* the graph is receiver-sorted with ``num_neighbors`` edges per receiver, the
  receiver itself first (distance 0).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import CgnnError
from .graph import Batch, Data

__all__ = ["extend_positions_torch", "generate_position_noise", "generate_temperature_noise", "preprocess",
           "preprocess_batch", "knn_graph_periodic"]


def _default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise CgnnError("no HIP device visible: cosmology_gnn_simulation_amd builds graphs on the GPU only")
    return torch.device("cuda", torch.cuda.current_device())


def extend_positions_torch(positions: torch.Tensor, box_size):
    """The 27-image extension of reference data_utils.py:9-33, kept for API
    compatibility (the engine itself never materialises it).  Returns
    ``(extended [N*3^d, d], mapping [N*3^d])``."""
    n, d = positions.shape
    if isinstance(box_size, list):
        box_size = float(box_size[0])
    axis = torch.tensor([-box_size, 0.0, box_size], device=positions.device, dtype=torch.float32)
    shifts = torch.cartesian_prod(*([axis] * d)).reshape(-1, d)
    extended = (positions.unsqueeze(0) + shifts.unsqueeze(1)).reshape(-1, d)
    mapping = torch.arange(n, device=positions.device).repeat(shifts.shape[0])
    return extended, mapping


def _wrap_displacement(d: torch.Tensor, box_size: float) -> torch.Tensor:
    half = box_size / 2
    d = torch.where(d < -1 * half, d + box_size, d)
    return torch.where(d > half, d - box_size, d)


def generate_position_noise(position_seq: torch.Tensor, noise_std: float, box_size: float, dt: float) -> torch.Tensor:
    """Random-walk position noise for ``[N, W, 3]`` (reference data_utils.py:36-54)."""
    p = position_seq.float()
    vel = _wrap_displacement(p[:, 1:] - p[:, :-1], box_size) / dt
    steps = vel.size(1)
    walk = (torch.randn_like(vel, dtype=torch.float32) * (noise_std / (steps ** 0.5))).cumsum(dim=1)
    pos_noise = walk.cumsum(dim=1) * dt
    return torch.cat((torch.zeros_like(pos_noise)[:, 0:1], pos_noise), dim=1)


def generate_temperature_noise(temperature_seq: torch.Tensor, noise_std: float, temp_rate_std, dt: float):
    """Random-walk temperature noise for ``[N, W, 1]`` (reference data_utils.py:57-70)."""
    t = temperature_seq.float()
    rate = (t[:, 1:] - t[:, :-1]) / dt
    steps = rate.size(1)
    walk = (torch.randn_like(rate, dtype=torch.float32) * (noise_std * temp_rate_std / (steps ** 0.5))).cumsum(dim=1)
    t_noise = walk.cumsum(dim=1) * dt
    return torch.cat((torch.zeros_like(t_noise)[:, 0:1], t_noise), dim=1)


def knn_graph_periodic(pos: torch.Tensor, box_size: float, k: int, want_order: bool = False, *,
                       min_image_edge_attr: bool = False, grid: str = "uniform"):
    """Periodic k-NN on the device.  Returns ``(edge_index int64 [2, N*k],
    edge_attr [N*k, 4], senders int32, order|None)``.  ``grid``, ``min_image_edge_attr``: as in ``ops.knn_periodic``."""
    ops.check_knn_grid(grid, "knn_graph_periodic")
    ops.check_min_image(min_image_edge_attr, "knn_graph_periodic")
    senders, edge_attr, order = ops.knn_periodic(pos, box_size, k, None, True, want_order, grid=grid,
                                                 min_image_edge_attr=min_image_edge_attr)
    n = pos.shape[0]
    receivers = torch.arange(n, device=pos.device, dtype=torch.int64).repeat_interleave(k)
    edge_index = torch.stack([senders.to(torch.int64), receivers], dim=0)
    return edge_index, edge_attr, senders, order


def _meta(metadata: dict, key: str, device) -> torch.Tensor:
    return torch.tensor(metadata[key], dtype=torch.float32, device=device)


def _draw_reference_noise(pos_seq: torch.Tensor, tmp_seq: torch.Tensor, noise_std: float, temp_rate_std, dt: float,
                          box_size: float):
    """The reference's two RNG draws (data_utils.py:47,:63) on the CPU generator.  ``randn_like`` follows the
    memory layout of its argument, so the draw order depends on the strides of the (permuted) windows; they are
    reproduced on zero-filled host tensors with the inputs' shapes and strides (the noise does not depend on the
    values), which spares device-resident windows a copy to the host."""
    def host_like(t):
        return t if not t.is_cuda else torch.empty_strided(t.shape, t.stride(), dtype=torch.float32).zero_()
    pos_noise = generate_position_noise(host_like(pos_seq), noise_std, box_size, dt)
    tmp_noise = generate_temperature_noise(host_like(tmp_seq), noise_std, temp_rate_std, dt)
    return pos_noise, tmp_noise


def preprocess(position_seq, temperature_seq, metadata, target_position=None, target_temperature=None,
               noise_std=0.0, num_neighbors=16, dt=None, box_size=None, device: Optional[torch.device] = None,
               reference_rng: bool = True, check_bounds: bool = True, noise_rng: str = "reference",
               noise_seed: Optional[int] = None, noise_draw: int = 0, *, min_image_edge_attr: bool = False,
               knn_grid: str = "uniform"):
    """Window ``[W, N, 3]`` / ``[W, N, 1]`` -> graph (reference data_utils.py:72-228).

    ``device`` (extension) selects the GPU; by default the inputs' device if they
    are already on one, else the current HIP device.  All returned tensors live
    there, so the caller's ``graph.to(device)`` is a no-op.  ``reference_rng=False``
    (extension, only honoured when ``noise_std == 0``) skips the two CPU random draws
    the reference makes even for zero noise; results are identical, only the global
    RNG stream is left untouched (used by the on-device rollout).  ``check_bounds=False`` (extension) drops the
    reference's sender-index assertion (:158-159), which costs one device-to-host synchronisation per call.

    ``noise_rng`` (extension) selects where the random-walk noise comes from.  ``"reference"`` (default) draws it on
    the CPU from torch's global generator with the reference's call sequence, bit for bit.  ``"device"`` makes it in
    the kernel that also forms ``x``, ``pos``, ``y_acc`` and ``y_temp_rate`` (``cgnn_training_sample``): a
    counter-based generator gives every (particle, time step) its four normals as a pure function of ``(noise_seed,
    noise_draw, particle id, step)``.  The noise then has the reference's distribution and the reference's arithmetic
    downstream of the normals, NOT its random stream: seeded comparisons against the reference stay on
    ``"reference"``.  The same ``(noise_seed, noise_draw)`` gives the same sample, so a training loop must pass a new
    ``noise_draw`` for every sample (``step * batch_size + i``); ``noise_seed=None`` means ``torch.initial_seed()``.
    The device path draws nothing on the CPU, leaves torch's global generator where it was, copies nothing from the
    host when the inputs live on the device, and does NOT add the noise into the caller's target tensors (the
    reference's in-place ``+=`` on them is a side effect of its host code, kept only on the ``"reference"`` path).

    ``knn_grid`` (extension): the cell grid of the neighbour search, ``"uniform"`` or ``"adaptive"``
    (``ops.knn_periodic``); the graph is the same bit for bit, ``"adaptive"`` builds it faster on clustered snapshots.

    ``min_image_edge_attr`` (extension, on both noise paths): ``False`` keeps the reference's edge features,
    ``pos[sender] - pos[receiver]``, which are about one box length long for every edge that crosses a box face;
    ``True`` writes the displacement to the periodic image the search ranked, and its norm (``ops.knn_periodic``).
    ``x``, ``edge_index``, ``pos`` and the targets do not depend on it."""
    ops.check_knn_grid(knn_grid, "preprocess")
    ops.check_min_image(min_image_edge_attr, "preprocess")
    if noise_rng not in ("reference", "device"):
        raise ValueError(f"noise_rng must be 'reference' or 'device', got {noise_rng!r}")
    dt = float(dt)
    box_size = float(box_size)
    if device is None:
        device = position_seq.device if position_seq.is_cuda else _default_device()
    device = torch.device(device)

    if noise_rng == "device":
        return _preprocess_device_noise(position_seq, temperature_seq, metadata, target_position, target_temperature,
                                        noise_std, int(num_neighbors), dt, box_size, device, check_bounds, noise_seed,
                                        noise_draw, knn_grid, min_image_edge_attr)

    pos_seq = position_seq.float().permute(1, 0, 2)                       # [N, W, 3]
    tmp_seq = temperature_seq.float()
    if tmp_seq.shape[0] == pos_seq.shape[1] and tmp_seq.shape[1] == pos_seq.shape[0]:
        tmp_seq = tmp_seq.permute(1, 0, 2)                                # [N, W, 1]
    if target_position is not None:
        target_position = target_position.float()

    # --- noise: drawn where the reference draws it (CPU RNG stream), then moved ---
    pos_noise_cpu = tmp_noise_cpu = None
    if reference_rng or noise_std != 0.0:
        trs_cpu = torch.tensor(metadata["temp_rate_std"], dtype=torch.float32)
        pos_noise_cpu, tmp_noise_cpu = _draw_reference_noise(pos_seq, tmp_seq, noise_std, trs_cpu, dt, box_size)

    pos_seq = pos_seq.to(device)                                          # [N, W, 3] view of the [W, N, 3] window
    tmp_seq = tmp_seq.to(device)
    pos_noise = tmp_noise = None
    if noise_std != 0.0:
        pos_noise, tmp_noise = pos_noise_cpu.to(device), tmp_noise_cpu.to(device)

    # --- node features and the wrapped last frame in one kernel (cgnn_window_features) ---
    node_features, recent_position = ops.window_features(pos_seq.permute(1, 0, 2), tmp_seq.permute(1, 0, 2), metadata, dt,
                                                         box_size, pos_noise, tmp_noise)

    velocity_seq = recent_temperature = None
    if target_position is not None or target_temperature is not None:
        # training targets (reference :166-214): the same element-wise expressions, on the device
        wp = torch.remainder(pos_seq + pos_noise, box_size) if noise_std != 0.0 else torch.remainder(pos_seq, box_size)
        velocity_seq = _wrap_displacement(wp[:, 1:] - wp[:, :-1], box_size) / dt
        recent_temperature = (tmp_seq + tmp_noise if noise_std != 0.0 else tmp_seq)[:, -1]

    if target_temperature is not None:
        target_temperature = target_temperature.float()
        if target_temperature.dim() == 3:
            target_temperature = target_temperature.permute(1, 0, 2).squeeze(1)
        elif target_temperature.dim() == 2 and target_temperature.shape[1] != 1:
            target_temperature = target_temperature.reshape(-1, 1)
        if target_temperature.shape != recent_temperature.shape and \
                target_temperature.numel() == recent_temperature.numel():
            target_temperature = target_temperature.reshape(recent_temperature.shape)

    # --- periodic k-NN graph + edge features on the device ---
    edge_index, edge_attr, senders, order = knn_graph_periodic(recent_position, box_size, int(num_neighbors),
                                                                want_order=True, grid=knn_grid,
                                                                min_image_edge_attr=min_image_edge_attr)
    n = recent_position.shape[0]
    if check_bounds:    # reference :158-159 (a host round trip: the on-device rollout turns it off)
        assert int(senders.max()) < n, f"Max sender index {int(senders.max())} >= {n}"

    acceleration = None
    temp_rate = None
    if target_position is not None:
        tp = target_position
        if tp.dim() == 3:
            tp = tp.permute(1, 0, 2).squeeze(1)
        elif tp.dim() == 2 and tp.shape[0] != n:
            tp = tp.reshape(-1, 3)
        if noise_std != 0.0:
            tp += pos_noise_cpu[:, -1].to(tp.device)   # in place on the caller's tensor, like the reference (:182)
        tp = tp.to(device)
        next_velocity = _wrap_displacement(tp - recent_position, box_size) / dt
        acceleration = (next_velocity - velocity_seq[:, -1]) / dt
        acceleration = (acceleration - _meta(metadata, "acc_mean", device)) / _meta(metadata, "acc_std", device)
    if target_temperature is not None:
        tt = target_temperature
        if tt.dim() == 3:
            tt = tt.squeeze(1)
        if noise_std != 0.0:
            tt += tmp_noise_cpu[:, -1].to(tt.device)   # in place, like the reference (:206)
        tt = tt.to(device)
        temp_rate = (tt - recent_temperature) / dt
        temp_rate = (temp_rate - _meta(metadata, "temp_rate_mean", device)) / _meta(metadata, "temp_rate_std", device)

    return _graph(node_features.float(), edge_index, edge_attr, acceleration.float() if acceleration is not None else None,
                  temp_rate.float() if temp_rate is not None else None, recent_position, order, dt, box_size,
                  int(num_neighbors), device)


def _graph(x, edge_index, edge_attr, y_acc, y_temp_rate, recent_position, order, dt: float, box_size: float, k: int,
           device) -> Data:
    graph = Data(
        x=x,
        edge_index=edge_index,
        edge_attr=edge_attr,
        y_acc=y_acc,
        y_temp_rate=y_temp_rate,
        pos=recent_position,
        dt=torch.full((1,), dt, dtype=torch.float32, device=device),            # (a fill kernel: torch.tensor([dt],
        box_size=torch.full((1,), box_size, dtype=torch.float32, device=device),  # device=...) would synchronise)
    )
    graph._cgnn_fixed_k = k
    graph._cgnn_fixed_k_for = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape))
    graph._cgnn_order = order          # spatial (cell-sorted) particle order: a locality hint for the engine
    return graph


def _batch_members(who: str, **named):
    """The per-simulation tensors of batched arguments: each is one tensor whose first dimension counts the B
    simulations, or a sequence of B tensors (ragged sizes); ``None`` stays ``None``.  All of them take the same form
    and agree on B >= 1.  -> (dict of lists, B).  Touches no device."""
    given = {name: v for name, v in named.items() if v is not None}
    whole = [name for name, v in given.items() if torch.is_tensor(v)]
    if whole and len(whole) != len(given):
        raise TypeError(f"{who}: {whole} are tensors and {sorted(set(given) - set(whole))} are sequences; a batch is "
                        f"either tensors with a leading batch dimension or sequences of per-simulation tensors")
    out, sizes = {}, {}
    for name, v in given.items():
        if torch.is_tensor(v) and v.dim() < 2:
            raise ValueError(f"{who}: {name} {tuple(v.shape)} has no batch dimension")
        members = list(v.unbind(0)) if torch.is_tensor(v) else list(v)
        if not all(torch.is_tensor(m) for m in members):
            raise TypeError(f"{who}: {name} must hold tensors")
        out[name], sizes[name] = members, len(members)
    if len(set(sizes.values())) != 1:
        raise ValueError(f"{who}: the arguments disagree on the number of simulations: {sizes}")
    b = next(iter(sizes.values()))
    if b < 1:
        raise ValueError(f"{who}: a batch holds at least one simulation")
    for name in named:
        out.setdefault(name, None)
    return out, b


def preprocess_batch(position_seqs, temperature_seqs, metadata, target_positions=None, target_temperatures=None,
                     noise_std=0.0, num_neighbors=16, dt=None, box_size=None, device: Optional[torch.device] = None,
                     noise_seed: Optional[int] = None, noise_draw: int = 0, *, min_image_edge_attr: bool = False,
                     knn_grid: str = "uniform") -> Batch:
    """B windows -> one ``Batch``: what ``Batch.from_data_list([preprocess(..., noise_rng="device", noise_draw=
    noise_draw + b, check_bounds=False) for b in range(B)])`` returns (the reference's batch, train.py:243-247), built
    with ONE neighbour search over all simulations (``ops.knn_periodic_batched``) and without the list form's second
    copy of every tensor.

    ``position_seqs``: ``[B, W, N, 3]``, or a sequence of B tensors ``[W, N_b, 3]`` (simulations of different sizes);
    ``temperature_seqs`` (``[W, N_b(, 1)]`` each) and the optional targets (``[N_b, 3]`` / ``[N_b(, 1)]`` each) take the
    same form.  Every simulation is a periodic box of side ``box_size`` and shares ``metadata`` and ``dt``.

    ``x``, ``edge_index``, ``edge_attr``, ``y_acc``, ``y_temp_rate``, ``pos``, ``dt``, ``box_size``, ``batch`` are equal
    to the list form's bit for bit, ``num_graphs`` and the fixed in-degree hint as well; the locality hint
    (``_cgnn_order``) is the batched search's own, block by block a cell-sorted order of each simulation.

    Noise is the device generator only (``noise_seed``, ``noise_draw`` as in ``preprocess``): simulation b is sampled by
    one ``cgnn_training_sample`` launch on its own window with draw ``noise_draw + b``, exactly the sample it gets alone.
    No host synchronisation.  ``knn_grid="adaptive"`` searches graph by graph (``ops.knn_periodic_batched``)."""
    who = "preprocess_batch"
    ops.check_knn_grid(knn_grid, who)
    ops.check_min_image(min_image_edge_attr, who)
    m, nb = _batch_members(who, position_seqs=position_seqs, temperature_seqs=temperature_seqs,
                           target_positions=target_positions, target_temperatures=target_temperatures)
    k, dt, box_size = int(num_neighbors), float(dt), float(box_size)
    offsets, w = [0], None
    for b, p in enumerate(m["position_seqs"]):
        if p.dim() != 3 or p.shape[2] != 3 or p.shape[1] < 1 or (w is not None and p.shape[0] != w):
            raise ValueError(f"{who}: window {b} must be [W, N, 3] with the batch's W, got {tuple(p.shape)}")
        w, n = int(p.shape[0]), int(p.shape[1])
        if m["temperature_seqs"][b].numel() != w * n:
            raise ValueError(f"{who}: temperature window {b} {tuple(m['temperature_seqs'][b].shape)} does not hold "
                             f"[{w}, {n}(, 1)]")
        if m["target_positions"] is not None and m["target_positions"][b].numel() != n * 3:
            raise ValueError(f"{who}: target_positions {b} {tuple(m['target_positions'][b].shape)} does not hold "
                             f"[{n}, 3]")
        if m["target_temperatures"] is not None and m["target_temperatures"][b].numel() != n:
            raise ValueError(f"{who}: target_temperatures {b} {tuple(m['target_temperatures'][b].shape)} does not "
                             f"hold {n} values")
        offsets.append(offsets[-1] + n)
    if device is None:
        first = m["position_seqs"][0]
        device = first.device if first.is_cuda else _default_device()
    device = torch.device(device)
    want = ["x", "recent_pos"] + (["y_acc"] if m["target_positions"] is not None else []) + \
        (["y_temp_rate"] if m["target_temperatures"] is not None else [])
    seed = torch.initial_seed() if noise_seed is None else int(noise_seed)
    samples = []
    for b in range(nb):
        n = offsets[b + 1] - offsets[b]
        tmp_w = m["temperature_seqs"][b].to(device)
        if tmp_w.dim() == 3 and tmp_w.shape[0] == n and tmp_w.shape[1] == w:
            tmp_w = tmp_w.permute(1, 0, 2)                                # [N, W, 1] -> [W, N, 1], as preprocess takes it
        tp = m["target_positions"][b].to(device).reshape(n, 3) if "y_acc" in want else None
        tt = m["target_temperatures"][b].to(device).reshape(n) if "y_temp_rate" in want else None
        samples.append(ops.training_sample(m["position_seqs"][b].to(device), tmp_w, metadata, dt, box_size,
                                           float(noise_std), seed % 2 ** 64, noise_draw + b, tp, tt, None, want))
    s = {name: torch.cat([smp[name] for smp in samples]) for name in want}
    recent = s["recent_pos"]
    senders, edge_attr, order = ops.knn_periodic_batched(recent, offsets, box_size, k, True, True,
                                                         min_image_edge_attr=min_image_edge_attr, grid=knn_grid)
    n_total = offsets[-1]
    receivers = torch.arange(n_total, device=device, dtype=torch.int64).repeat_interleave(k)
    y_tr = s.get("y_temp_rate")
    out = Batch(x=s["x"], edge_index=torch.stack([senders.to(torch.int64), receivers], dim=0), edge_attr=edge_attr,
                y_acc=s.get("y_acc"), y_temp_rate=y_tr.reshape(n_total, 1) if y_tr is not None else None, pos=recent,
                dt=torch.full((nb,), dt, dtype=torch.float32, device=device),
                box_size=torch.full((nb,), box_size, dtype=torch.float32, device=device),
                batch=batch_vector(offsets, device), num_graphs=nb)
    out._cgnn_fixed_k = k
    out._cgnn_fixed_k_for = (out.edge_index.data_ptr(), out.edge_index._version, tuple(out.edge_index.shape))
    out._cgnn_order = order
    return out


def batch_vector(offsets, device) -> torch.Tensor:
    """``batch[i]`` = the graph of row i (int64 ``[offsets[-1]]``), as ``Batch.from_data_list`` writes it: one fill per
    graph, nothing copied from the host."""
    return torch.cat([torch.full((b - a,), g, dtype=torch.long, device=device)
                      for g, (a, b) in enumerate(zip(offsets, offsets[1:]))])


def _preprocess_device_noise(position_seq, temperature_seq, metadata, target_position, target_temperature, noise_std,
                             k: int, dt: float, box_size: float, device, check_bounds: bool, noise_seed, noise_draw,
                             knn_grid: str = "uniform", min_image_edge_attr: bool = False):
    """``preprocess(noise_rng="device")``: one launch for noise, features, last frame and targets, then the k-NN."""
    n = position_seq.shape[1]
    pos_w = position_seq.to(device)                                       # [W, N, 3], as the kernel reads it
    tmp_w = temperature_seq.to(device)
    if tmp_w.dim() == 3 and tmp_w.shape[0] == n and tmp_w.shape[1] == pos_w.shape[0]:
        tmp_w = tmp_w.permute(1, 0, 2)                                    # [N, W, 1] -> [W, N, 1]
    want = ["x", "recent_pos"]
    if target_position is not None:
        if target_position.numel() != n * 3:
            raise CgnnError(f"preprocess: target_position {tuple(target_position.shape)} does not hold [N, 3]")
        target_position = target_position.to(device).reshape(n, 3)       # [N, 3] or [1, N, 3]
        want.append("y_acc")
    if target_temperature is not None:
        if target_temperature.numel() != n:
            raise CgnnError(f"preprocess: target_temperature {tuple(target_temperature.shape)} does not hold N values")
        target_temperature = target_temperature.to(device).reshape(n)    # [N], [N, 1] or [1, N, 1]
        want.append("y_temp_rate")
    seed = torch.initial_seed() if noise_seed is None else int(noise_seed)
    s = ops.training_sample(pos_w, tmp_w, metadata, dt, box_size, float(noise_std), seed % 2 ** 64, noise_draw,
                            target_position, target_temperature, None, want)
    recent_position = s["recent_pos"]
    edge_index, edge_attr, senders, order = knn_graph_periodic(recent_position, box_size, k, want_order=True,
                                                                grid=knn_grid,
                                                                min_image_edge_attr=min_image_edge_attr)
    if check_bounds:    # reference :158-159 (a host round trip)
        assert int(senders.max()) < n, f"Max sender index {int(senders.max())} >= {n}"
    y_tr = s.get("y_temp_rate")
    return _graph(s["x"], edge_index, edge_attr, s.get("y_acc"), y_tr.reshape(n, 1) if y_tr is not None else None,
                  recent_position, order, dt, box_size, k, device)
