"""Torch restatements for AttMIL's bf16 compute mode and the typed pooling kernels (data-free helpers;
the tests that use them are test_attmil_bf16_cpu.py and test_attmil_bf16_gpu.py).

``pool_ref``          gated attention pooling forward and backward in fp64 (autograd), from
                      Z [N, 2D], H [N, L], w [1, D], b [1], Wc [C, L], bc [C], dlogits [1, C] to
                      a, M, logits, dZ, dH_pool (= p_i dM: Z is an independent input here, as it is
                      for the kernels), dw, db, dWc, dbc.
``bf16_forward_ref``  the bf16 mode's model forward on the CPU with the implementation's rounding
                      points: the bag and the weights of ``_fc1``'s Linears and of the gate layer are
                      rounded to bf16 before each product (fp32 products and sums), LayerNorm reads
                      fp32 and its output is rounded to bf16, the 2048 branch's H = GELU(..) is rounded to
                      bf16, Z is rounded to bf16; biases, GELU, LayerNorm statistics, scores, softmax, M
                      and the classifier are fp32.  Eval mode (Dropout is the identity).
"""
import torch
import torch.nn.functional as F


def pool_ref(Z, H, w, b, Wc, bc, dlogits):
    Z, H, w, b, Wc, bc = (t.detach().double().clone().requires_grad_(True) for t in (Z, H, w, b, Wc, bc))
    D = Z.shape[1] // 2
    a = (torch.tanh(Z[:, :D]) * torch.sigmoid(Z[:, D:])) @ w.reshape(1, D).T + b      # [N, 1]
    p = torch.softmax(a.T, dim=1)                                                     # [1, N]
    M = p @ H                                                                         # [1, L]
    logits = M @ Wc.T + bc
    (logits * dlogits.double().reshape(1, -1)).sum().backward()
    return dict(a=a.detach().reshape(-1), M=M.detach().reshape(-1), logits=logits.detach(), dZ=Z.grad, dH_pool=H.grad,
                dw=w.grad.reshape(1, D), db=b.grad.reshape(1), dWc=Wc.grad, dbc=bc.grad)


def rb(t):
    """Round to bf16 (nearest even), back in fp32."""
    return t.float().bfloat16().float()


def bf16_forward_ref(model, x):
    """``model``: an AttMIL (ours or the oracle's: same module layout) with fp32 parameters on the CPU;
    x [1, N, F] or [N, F].  Returns logits [1, C] fp32."""
    with torch.no_grad():
        f = model._fc1
        x = x.reshape(-1, x.shape[-1])
        y0 = F.gelu(rb(x) @ rb(f[0].weight).T + f[0].bias.float())
        ln = f[3]
        h = rb(F.layer_norm(y0, (y0.shape[1],), ln.weight.float(), ln.bias.float(), ln.eps))
        if len(f) == 6:
            h = rb(F.gelu(h @ rb(f[4].weight).T + f[4].bias.float()))
        V, U = model.attention_V[0], model.attention_U[0]
        zv = rb(h @ rb(V.weight).T + V.bias.float())
        zu = rb(h @ rb(U.weight).T + U.bias.float())
        a = (torch.tanh(zv) * torch.sigmoid(zu)) @ model.attention_weights.weight.float().T \
            + model.attention_weights.bias.float()
        p = torch.softmax(a.T, dim=1)
        c = model.classifier[0]
        return (p @ h) @ c.weight.float().T + c.bias.float()
