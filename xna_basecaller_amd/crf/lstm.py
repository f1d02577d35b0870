"""
One LSTM layer of the encoder as a torch autograd function: `model.encoder[i](x)` on a device tensor returns a tensor with a
grad_fn (crf/model.py:LSTM.forward).  The recurrence -- T dependent steps forward, T backward -- runs in
xb_lstm_train_forward_dev / xb_lstm_train_backward_dev on the tensors' own memory; the products without a recurrence are
torch's: gin = x W_ih^T + b before the function (so autograd supplies dx, dW_ih and db from dgin), and
dW_hh = sum_t dgin[t]^T h_prev[t] inside its backward, one matmul on the shifted y.
"""
import torch


class _LstmRecurrence(torch.autograd.Function):
    """(gin (T, n, 4F), w_hh (4F, F), reverse, ctx) -> y (T, n, F); saves the activated gates, the cell states and y."""

    @staticmethod
    def forward(fctx, gin, w_hh, reverse, ctx):
        T, n, G = gin.shape
        F = G // 4
        gin, w_hh = gin.contiguous(), w_hh.contiguous()
        y = torch.empty((T, n, F), dtype=torch.float32, device=gin.device)
        gates = torch.empty((T, n, G), dtype=torch.float32, device=gin.device)
        c = torch.empty((T, n, F), dtype=torch.float32, device=gin.device)
        torch.cuda.current_stream(gin.device).synchronize()      # the inputs are written; the context's stream may read them
        ctx.lstm_train_forward_dev(gin.data_ptr(), w_hh.data_ptr(), T, n, F, reverse, y.data_ptr(), gates.data_ptr(), c.data_ptr())
        ctx.synchronize()                                        # ... and torch's stream the outputs
        fctx.save_for_backward(w_hh, gates, c, y)
        fctx.reverse, fctx.ctx = bool(reverse), ctx
        return y

    @staticmethod
    def backward(fctx, dy):
        w_hh, gates, c, y = fctx.saved_tensors
        T, n, F = y.shape
        dy = dy.to(torch.float32).contiguous()
        dgin = torch.empty_like(gates)
        torch.cuda.current_stream(dy.device).synchronize()
        fctx.ctx.lstm_train_backward_dev(dy.data_ptr(), w_hh.data_ptr(), gates.data_ptr(), c.data_ptr(), T, n, F, fctx.reverse,
                                         dgin.data_ptr())
        fctx.ctx.synchronize()
        dw_hh = None
        if fctx.needs_input_grad[1]:
            # h_prev[t] is y of the step processed before t, zero at the first: the sum skips that step
            d, h = (dgin[:-1], y[1:]) if fctx.reverse else (dgin[1:], y[:-1])
            dw_hh = torch.matmul(d.reshape(-1, 4 * F).t(), h.reshape(-1, F))
        return dgin, dw_hh, None, None


def lstm_forward(layer, x):
    """crf.model.LSTM.forward: the checks, the input projection (torch) and the recurrence (device kernels)."""
    model = getattr(layer, "_model", None)
    model = model() if model is not None else None
    if model is None:
        raise RuntimeError("LSTM.forward runs on the device context of a Model: call it as model.encoder[i](x), not on a layer "
                           "built on its own")
    if not isinstance(x, torch.Tensor) or not x.is_cuda or (x.device.index or 0) != model._device:
        raise ValueError("LSTM.forward takes a torch tensor on the model's device cuda:%d, got %s: pass x.to('cuda:%d')"
                         % (model._device, x.device if isinstance(x, torch.Tensor) else type(x).__name__, model._device))
    if x.dtype != torch.float32:
        raise TypeError("LSTM.forward takes float32, got %s: pass x.to(torch.float32)" % x.dtype)
    rnn = layer.rnn
    if x.dim() != 3 or x.shape[2] != rnn.input_size:
        raise ValueError("LSTM.forward takes (T, N, %d), got %s" % (rnn.input_size, tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError("LSTM.forward takes a contiguous tensor: pass x.contiguous()")
    if rnn.weight_hh_l0.device != x.device:
        raise ValueError("LSTM.forward: the layer's parameters are on %s, x on %s: move the layer first, model.encoder[i].to('%s')"
                         % (rnn.weight_hh_l0.device, x.device, x.device))
    T, N, _ = x.shape
    ctx = model.context(T * model.stride, N)
    gin = torch.nn.functional.linear(x, rnn.weight_ih_l0, rnn.bias_ih_l0 + rnn.bias_hh_l0)
    return _LstmRecurrence.apply(gin, rnn.weight_hh_l0, layer.reverse, ctx)
