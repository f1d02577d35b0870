"""
Fine-tuning of the CRF head with the encoder below it frozen -- `bonito train -F` at --num-unfreeze-top 1
(ub-bonito/bonito/cli/train.py:134-158, training.py:91-117): the one layer with trainable parameters is LinearCRFEncoder
(encoder.9.linear.{weight,bias}), so a step needs no backward pass through the recurrence.  HeadTrainer owns the device
state of such a run on the model's context (xb_head_train_begin .. xb_head_train_end): fp32 master weights, AdamW's moments,
the step count.  A step is one device call (xb_head_train_step): encoder, loss gradient, head gradient, norm, clipping at 2.0,
AdamW with torch's defaults, re-pack; nothing score-sized leaves the device.
"""
from collections import OrderedDict

import torch

W_KEY, B_KEY = "encoder.9.linear.weight", "encoder.9.linear.bias"


class HeadTrainer:

    def __init__(self, model, chunk_len, batch):
        last = model.encoder[-1]
        if getattr(last, "scale", None) is None or not float(last.scale) > 0:
            raise NotImplementedError("the head trainer needs the head's scale (scores = scale * tanh(Wx + b)); this model has none")
        self.model = model
        self.ctx = model.context(chunk_len, batch)
        self.chunk_len, self.max_batch = int(chunk_len), self.ctx.max_batch
        self.ctx.head_train_begin(last.linear.weight.detach().to(torch.float32).cpu().numpy(),
                                  last.linear.bias.detach().to(torch.float32).cpu().numpy())
        self.steps = 0

    def _live(self):
        if self.ctx is None or self.model._ctx is not self.ctx:
            raise RuntimeError("the head trainer's device context is gone (the model was moved, reloaded or asked for another "
                               "chunk length or a larger batch): create a new trainer")

    def step(self, batch, targets, lengths, lr):
        """One optimiser step on a (N,1,L) batch with its (N,Lt) label rows and (N,) lengths at learning rate lr ->
        (mean loss before the step, gradient norm before clipping)."""
        self._live()
        sig = self.model._as_signal(batch)
        if sig.shape[1] != self.chunk_len or sig.shape[0] > self.max_batch:
            raise ValueError("batch of %d chunks of %d samples: this trainer takes up to %d chunks of %d"
                             % (sig.shape[0], sig.shape[1], self.max_batch, self.chunk_len))
        out = self.ctx.head_train_step(sig, targets, lengths, lr)
        self.steps += 1
        return out

    def weights(self):
        self._live()
        return self.ctx.head_get_weights()

    def state_dict(self):
        """The model's state dict with the two head tensors replaced by the trained ones."""
        w, b = self.weights()
        sd = OrderedDict((k, v.detach().clone()) for k, v in self.model.state_dict().items())
        sd[W_KEY] = torch.from_numpy(w).to(sd[W_KEY].dtype)
        sd[B_KEY] = torch.from_numpy(b).to(sd[B_KEY].dtype)
        return sd

    def close(self):
        """End the run: the trained floats go into the model's own parameters (its live context already computes with them)."""
        if self.ctx is None:
            return
        self._live()
        w, b = self.ctx.head_get_weights()
        self.ctx.head_train_end()
        last = self.model.encoder[-1]
        with torch.no_grad():
            last.linear.weight.copy_(torch.from_numpy(w))
            last.linear.bias.copy_(torch.from_numpy(b))
        self.ctx = None
