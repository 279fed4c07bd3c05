"""flow_encoder[0] (7x7, 4 -> 128) stand-alone at the bench shape: fp32-map kernel against the padded-fp16 kernel, and the
whole encoder as one launch (glorie_flow_encoder) against its two launches.
python tools/bench_flow.py  (FLOW_N = maps)"""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glorie_slam_amd import update_ops as U

dev = torch.device("cuda:0")
n, h, w = int(os.environ.get('FLOW_N', '36')), 60, 80
torch.manual_seed(0)
flow = torch.randn(n, h, w, 4, device=dev)
wgt = torch.randn(128, 4, 7, 7, device=dev) / 14
bias = torch.randn(128, device=dev)
wp = U.pack_flow_conv7(wgt)
out = torch.empty((n, 128, h, w), dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
out2 = torch.empty_like(out)
pf = U.PaddedFlow(n, h, w, dev)
U.flow_pad(flow, pf)
ref = torch.relu(torch.nn.functional.conv2d(flow.permute(0, 3, 1, 2).half().float(), wgt.half().float(), bias, padding=3))


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


t0 = timed(lambda: U.flow_conv7(flow, wp, bias, out))
t1 = timed(lambda: U.flow_conv7_padded(pf, wp, bias, out2))
t2 = timed(lambda: U.flow_pad(flow, pf))
print("fp32 map %.1f us (err %.4f)   padded fp16 %.1f us (err %.4f, equal to fp32-map kernel: %s)   pad pass %.1f us" % (
    t0, float((out.float() - ref).abs().max()), t1, float((out2.float() - ref).abs().max()), bool(torch.equal(out, out2)), t2))

# the whole encoder: one launch (hidden map in LDS) against flow_conv7_padded + conv_igemm, into the step's channel slice
wgt3 = torch.randn(64, 128, 3, 3, device=dev) / 34
bias3 = torch.randn(64, device=dev)
w3 = U.pack_conv_igemm(wgt3, pair=True)
hx_a = torch.zeros((n, 320, h, w), dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
hx_b = torch.zeros_like(hx_a)


def two_launches():
    U.flow_conv7_padded(pf, wp, bias, out2)
    U.conv_igemm(out2, None, w3, 9, 64, hx_a[:, 256:320], terms=bias3, act=U.ACT_RELU)


t3 = timed(two_launches)
t4 = timed(lambda: U.conv_igemm(out2, None, w3, 9, 64, hx_a[:, 256:320], terms=bias3, act=U.ACT_RELU))
t5 = timed(lambda: U.flow_encoder(pf, wp, bias, w3, bias3, hx_b[:, 256:320]))
print("flow encoder %dx%dx%d: two launches %.1f us (7x7 %.1f + 3x3 %.1f alone)   one launch %.1f us   torch.equal: %s" % (
    n, h, w, t3, t1, t4, t5, bool(torch.equal(hx_a, hx_b))))
