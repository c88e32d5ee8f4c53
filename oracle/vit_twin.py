"""Float64 twin of MyViT (phase1_lifting/baselineModel.py:220-362) in plain torch on the CPU.  TEST INFRASTRUCTURE ONLY.

Written from the model's definition with stock torch ops (no import of the package or the reference): the GPU tests
compare the HIP forward and backward against it.

    params(sd)                 float64 leaf copies of a state_dict (pos_embed without a gradient, unless asked)
    forward(p, x)              the model's forward on those leaves; differentiable in p and in x
    grads(p)                   {name: gradient} of the leaves that received one
    twin(sd, x, t=None, ...)   one forward + backward: MSE against t, or an upstream gradient dy

forward() composes: a caller can chain two models (proj(lift(x))) or call one model twice in one graph and run one
backward over the sum, as phase5_loop/train_5.py does.
"""
import torch
import torch.nn.functional as F

DIM_HEAD = 64
EPS = 1e-5


def params(sd, requires_grad=True, pos_grad=False):
    """float64 CPU leaves of a state_dict; pos_embed requires a gradient only with pos_grad (the model's default)."""
    return {k: v.detach().double().cpu().clone().requires_grad_(requires_grad and (pos_grad or k != "pos_embed"))
            for k, v in sd.items()}


def n_blocks(p):
    return len({k.split(".")[1] for k in p if k.startswith("blocks.")})


def forward(p, x, n_heads=None):
    """y [B][seq][out_d] of the model with parameters p (params()) on x [B][seq][in_d] (any dtype: computed in float64)."""
    H = p["linear_mapper.weight"].shape[0]
    heads = H // DIM_HEAD if n_heads is None else n_heads
    x = torch.as_tensor(x)
    x = x.double() if x.dtype != torch.float64 else x
    B, n, _ = x.shape
    h = x @ p["linear_mapper.weight"].T + p["linear_mapper.bias"] + p["pos_embed"]
    for i in range(n_blocks(p)):
        q_ = f"blocks.{i}."
        a = F.layer_norm(h, (H,), p[q_ + "norm1.weight"], p[q_ + "norm1.bias"], EPS)
        a = F.layer_norm(a, (H,), p[q_ + "mhsa.norm.weight"], p[q_ + "mhsa.norm.bias"], EPS)
        q, k, v = (a @ p[q_ + "mhsa.to_qkv.weight"].T).chunk(3, dim=-1)
        q, k, v = (z.reshape(B, n, heads, H // heads).transpose(1, 2) for z in (q, k, v))
        att = torch.softmax((q @ k.transpose(-1, -2)) * (H // heads) ** -0.5, dim=-1)
        o = (att @ v).transpose(1, 2).reshape(B, n, H)
        h = h + o @ p[q_ + "mhsa.to_out.weight"].T
        n2 = F.layer_norm(h, (H,), p[q_ + "norm2.weight"], p[q_ + "norm2.bias"], EPS)
        u = F.gelu(F.linear(n2, p[q_ + "mlp.0.weight"], p[q_ + "mlp.0.bias"]))
        h = h + F.linear(u, p[q_ + "mlp.2.weight"], p[q_ + "mlp.2.bias"])
    return F.linear(torch.relu(F.linear(h, p["mlp.0.weight"], p["mlp.0.bias"])), p["mlp.2.weight"], p["mlp.2.bias"])


def mse(y, t):
    return ((y - torch.as_tensor(t).double()) ** 2).mean()


def grads(p):
    return {k: v.grad.numpy() for k, v in p.items() if v.grad is not None}


def twin(sd, x, t=None, n_heads=None, dy=None, x_grad=False):
    """Forward + backward of the model in float64: the loss is MSE(y, t), or y is backpropagated with the upstream
    gradient dy.  Returns (y, {name: grad}), and the input gradient third when x_grad."""
    p = params(sd)
    x = torch.as_tensor(x).double().clone().requires_grad_(x_grad)
    y = forward(p, x, n_heads)
    if dy is None:
        mse(y, t).backward()
    else:
        y.backward(torch.as_tensor(dy).double())
    out = (y.detach().numpy(), grads(p))
    return out + (x.grad.numpy(),) if x_grad else out
