"""
The training criterion as a torch autograd function: CTC_CRF.ctc_loss on scores that are a torch tensor on the model's device
(training.py:82 takes model.seqdist.ctc_loss as Trainer's criterion; the reference's is seqdist's, CUDA-only).  The forward runs
xb_ctc_loss_grad_dev on the tensors' own memory -- loss and d loss / d scores in one device call -- and saves the gradient; the
backward is a product.  No backward through the encoder: torch's own layers provide that (the head alone is trained without
torch: crf/trainer.py).
"""
import torch


def _check_scores(seqdist, scores):
    nb, S = seqdist.n_base, seqdist.n_base ** seqdist.state_len
    if scores.dtype != torch.float32:
        raise TypeError("ctc_loss on the device takes float32 scores, got %s (AMP: cast with scores.to(torch.float32), as "
                        "training.py:99 does)" % scores.dtype)
    if scores.dim() != 3 or scores.shape[2] not in (S * (nb + 1), S * nb):
        raise ValueError("ctc_loss on the device takes (T, N, %d) or (T, N, %d) scores, got %s"
                         % (S * (nb + 1), S * nb, tuple(scores.shape)))
    if not scores.is_contiguous():
        raise ValueError("ctc_loss on the device takes contiguous scores: call scores.contiguous()")
    return scores.shape[2] == S * (nb + 1)


class _CtcLossGrad(torch.autograd.Function):
    @staticmethod
    def forward(fctx, scores, targets, target_lengths, ctx, has_blank, loss_clip, reduction):
        T, N, _ = scores.shape
        dev = scores.device
        targets = torch.as_tensor(targets).to(device=dev, dtype=torch.uint8).contiguous()
        lengths = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int32).contiguous()
        if targets.dim() != 2 or targets.shape[0] != N or lengths.shape != (N,):
            raise ValueError("ctc_loss: targets (N, Lt) and target_lengths (N) expected for scores (T, N, C)")
        loss = torch.empty((N,), dtype=torch.float32, device=dev)
        grad = torch.empty_like(scores)
        torch.cuda.current_stream(dev).synchronize()             # the inputs are written; the context's stream may read them
        ctx.ctc_loss_grad_dev(scores.data_ptr(), T, N, has_blank, targets.data_ptr(), targets.shape[1], lengths.data_ptr(),
                              loss.data_ptr(), grad.data_ptr(), loss_clip=loss_clip, reduction=reduction)
        ctx.synchronize()                                        # ... and torch's stream the outputs; bad labels surface here
        fctx.save_for_backward(grad)
        fctx.mean = reduction == "mean"
        return loss.mean() if fctx.mean else loss

    @staticmethod
    def backward(fctx, grad_output):
        grad, = fctx.saved_tensors
        if fctx.mean:
            return (grad * grad_output,) + (None,) * 6
        return (grad * grad_output.to(grad.dtype)[None, :, None],) + (None,) * 6


def ctc_loss(seqdist, model, scores, targets, target_lengths, loss_clip=None, reduction="mean", normalise_scores=True):
    """CTC_CRF.ctc_loss for a torch tensor of RAW scores on the model's device: a tensor with a grad_fn (scalar for 'mean',
    (N,) for 'none')."""
    if not normalise_scores:
        raise NotImplementedError("normalise_scores=False has no device path: pass numpy scores (CTC_CRF.ctc_loss(numpy, ..., "
                                  "normalise_scores=False, want_grad=True))")
    if reduction not in ("mean", "none", None):
        raise ValueError("Unknown reduction type {}".format(reduction))
    if not scores.is_cuda or (scores.device.index or 0) != model._device:
        raise ValueError("ctc_loss: scores on %s, the model is on cuda:%d" % (scores.device, model._device))
    has_blank = _check_scores(seqdist, scores)
    T, N, _ = scores.shape
    ctx = model.context(T * model.stride, N)
    return _CtcLossGrad.apply(scores, targets, target_lengths, ctx, has_blank, loss_clip, "mean" if reduction == "mean" else "none")
