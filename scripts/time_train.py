"""Developer tool: time one training step (forward + backward + Adam) through the HIP node-stream kernels and
print the per-op split (HIP events on the launch stream).  Not part of the product or tests.
    python scripts/time_train.py [--particles 1000000] [--latent 128] [--mp-steps 10]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosmology_gnn_simulation_amd import data_utils, graph_network, losses, ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=1_000_000)
ap.add_argument("--neighbors", type=int, default=16)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--mp-steps", type=int, default=10)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--train-precision", default="fp32", choices=["fp32", "fp32x3"])
ap.add_argument("--hidden", type=int, default=None, help="mlp_hidden_size (default: the latent size)")
ap.add_argument("--with-edge-stream", action="store_true",
                help="also run the edge stream's forward (model.train_edge_stream): under the reference nothing reads it "
                     "(SURVEY F1) but its step computes it -- the like-for-like step time")
ap.add_argument("--message-source", default="x_j", choices=["x_j", "edge"],
                help="edge: train the Interaction Network that aggregates the edge updates (model.train_edge_messages)")
ap.add_argument("--noise-std", type=float, default=0.0,
                help="> 0: rebuild the training sample inside every timed step with noise made on the device "
                     "(preprocess(noise_rng='device'), windows resident on the GPU, a new draw per step)")
a = ap.parse_args()
dev = "cuda"
n, k, d, L = a.particles, a.neighbors, a.latent, a.mp_steps
snap = synthetic.make_snapshot(n, seed=1236)
meta = synthetic.make_metadata()
c, e = snap["Coordinates"], snap["InternalEnergy"]
g = data_utils.preprocess(c[:5], e[:5], meta, c[5], e[5], 0.0, k, 0.01, 1.0)
hd = a.hidden or d
m = graph_network.EncodeProcessDecode(d, hd, 2, L, 3)
m.load_state_dict(synthetic.make_state_dict(d, hd, 2, L, 3))
m = m.to(dev).train()
m.train_precision = a.train_precision
m.train_edge_stream = a.with_edge_stream
m.message_source = a.message_source
m.train_edge_messages = a.message_source == "edge"
if a.with_edge_stream:
    m.edge_precision, m.node_precision = "bf16", "fp16x2"      # bench.py's edge stream
opt = torch.optim.Adam(m.parameters(), lr=1e-4)
mse = torch.nn.functional.mse_loss
if a.noise_std > 0:
    c, e = c.to(dev), e.to(dev)
draws = 0


def step():
    global g, draws
    if a.noise_std > 0:
        g = data_utils.preprocess(c[:5], e[:5], meta, c[5], e[5], a.noise_std, k, 0.01, 1.0, check_bounds=False,
                                  noise_rng="device", noise_seed=1236, noise_draw=draws)
        draws += 1
    pred = m(g)
    loss = (mse(pred["acceleration"], g.y_acc) + mse(pred["temp_rate"], g.y_temp_rate)
            + losses.momentum_conservation_loss(pred["acceleration"], g, 0.01, 0.1))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


for _ in range(2):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.iters):
    step()
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / a.iters * 1e3
what = ("message_source edge (both streams differentiated)" if a.message_source == "edge" else
        "edge stream forward included" if a.with_edge_stream else "edge stream skipped (F1)")
if a.noise_std > 0:
    what += f"; sample rebuilt in the step with device noise, noise_std {a.noise_std:g}"
print(f"training step ({what}, {a.train_precision}): {ms:.2f} ms  "
      f"({n} particles, k={k}, latent {d}, hidden {hd}, {L} rounds; "
      f"{n * k * L / ms / 1e6:.3f} G edge-updates/s)", flush=True)
with ops.OpTimer() as tm:
    step()
for name, (calls, total) in sorted(tm.summary().items(), key=lambda kv: -kv[1][1]):
    print(f"  {name:16s} {calls:4d} calls {total:9.3f} ms", flush=True)
print(f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
if a.message_source == "edge":      # cgnn_edge_mlp_backward per call against its byte and matrix floors
    ne, H, nh = n * k, hd, 2
    calls, total = tm.summary().get("edge_mlp_backward", (0, 0.0))
    if calls:
        per = total / calls
        # read e, de_in, d_agg rows, P rows; write h, g_a (nh each), g_o, zhat, dy, de_out
        nbytes = 4 * ne * (2 * d + 2 * H + 2 * nh * H + 4 * d)
        flops = 2 * ne * (2 * (d * H + (nh - 1) * H * H + H * d) + H * d)     # recompute + data gradient
        print(f"  edge_mlp_backward {per:.3f} ms per call: {nbytes / 1e9:.2f} GB -> byte floor {nbytes / 6.3e12 * 1e3:.3f} ms "
              f"at 6.3 TB/s; {flops / 1e12:.3f} TFLOP -> matrix floor {flops / 157e12 * 1e3:.3f} ms (f32 MFMA, 157 TFLOP/s)")
