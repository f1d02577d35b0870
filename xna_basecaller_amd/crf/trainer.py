"""
Fine-tuning of the CRF head with the encoder below it frozen -- `bonito train -F` at --num-unfreeze-top 1
(ub-bonito/bonito/cli/train.py:134-158, training.py:91-117): the one layer with trainable parameters is LinearCRFEncoder
(encoder.9.linear.{weight,bias}), so a step needs no backward pass through the recurrence.  HeadTrainer owns the device
state of such a run on the model's context (xb_head_train_begin .. xb_head_train_end): fp32 master weights, AdamW's moments,
the step count.  A step is one device call (xb_head_train_step): encoder, loss gradient, head gradient, norm, clipping at 2.0,
AdamW with torch's defaults, re-pack; nothing score-sized leaves the device.

TopTrainer is the same run with the top L = K - 1 LSTM layers unfrozen beside the head (--num-unfreeze-top K in 2 .. 6 with
--no-amp: float32 throughout above the frozen bottom).  Its step is one device call too (xb_top_train_step): the inference
encoder's bottom pass, the training recurrences and fp32 products forwards and backwards, the loss gradient, one norm, one
clipped AdamW update over all 4 L + 2 tensors.  The step reads fp32 master weights that only the trainer holds; the packed
forms the inference path reads change when publish() loads the masters into the live context (once per epoch).

FullTrainer is TopTrainer with every key of the state dict: `train --no-amp` without -F, the reference's recipe that freezes
nothing.  The step (xb_full_train_begin, then the same xb_top_train_step) runs the three convolutions in their float32 training
form in place of the inference bottom, all five LSTM layers, the head, and the convolutions' backward behind the lowest layer's.

What the three share is Trainer: the run's life on the model's context, the step, the checkpoint, publish() and close().  A
trainer says which keys it trains (_keys), how the device run begins and ends (_begin, _end), what a step calls (_step) and how
the masters come back (_masters).
"""
from collections import OrderedDict

import numpy as np
import torch

W_KEY, B_KEY = "encoder.9.linear.weight", "encoder.9.linear.bias"
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
CONV_KEYS = tuple("encoder.%d.conv.%s" % (n, k) for n in range(3) for k in ("weight", "bias"))


def top_keys(layers):
    """The state-dict keys a TopTrainer of `layers` LSTM layers trains, in the order of csrc/xb_top_plan.h."""
    return ["encoder.%d.rnn.%s" % (n, k) for n in range(9 - layers, 9) for k in LSTM_KEYS] + [W_KEY, B_KEY]


def full_keys():
    """The state-dict keys a FullTrainer trains, in the order of csrc/xb_conv_plan.h and xb_top_plan.h: all 28."""
    return list(CONV_KEYS) + top_keys(5)


class Trainer:
    # the step leaves the inference forms of the live context as they were: publish() has to load the masters into them
    reloads = True

    def __init__(self, model, chunk_len, batch):
        last = model.encoder[-1]
        if getattr(last, "scale", None) is None or not float(last.scale) > 0:
            raise NotImplementedError("the trainer needs the head's scale (scores = scale * tanh(Wx + b)); this model has none")
        self.model = model
        self.keys = list(self._keys())
        self.ctx = model.context(chunk_len, batch)
        self.chunk_len, self.max_batch = int(chunk_len), self.ctx.max_batch
        sd = model.state_dict()
        self.shapes = [tuple(sd[k].shape) for k in self.keys]
        self._begin([sd[k].detach().to(torch.float32).cpu().numpy() for k in self.keys])
        self.steps = 0

    def _live(self):
        if self.ctx is None or self.model._ctx is not self.ctx:
            raise RuntimeError("the trainer's device context is gone (the model was moved, reloaded or asked for another "
                               "chunk length or a larger batch): create a new trainer")

    def _signal(self, batch):
        self._live()
        sig = self.model._as_signal(batch)
        if sig.shape[1] != self.chunk_len or sig.shape[0] > self.max_batch:
            raise ValueError("batch of %d chunks of %d samples: this trainer takes up to %d chunks of %d"
                             % (sig.shape[0], sig.shape[1], self.max_batch, self.chunk_len))
        return sig

    def step(self, batch, targets, lengths, lr):
        """One optimiser step on a (N,1,L) batch with its (N,Lt) label rows and (N,) lengths at learning rate lr ->
        (mean loss before the step, gradient norm before clipping)."""
        out = self._step(self._signal(batch), targets, lengths, lr)
        self.steps += 1
        return out

    def weights(self):
        """The master weights: key -> float32 array in the tensor's own shape."""
        self._live()
        return OrderedDict((k, np.array(a).reshape(shape)) for k, a, shape in zip(self.keys, self._masters(), self.shapes))

    def state_dict(self):
        """The model's state dict with the trained tensors replaced by the masters."""
        sd = OrderedDict((k, v.detach().clone()) for k, v in self.model.state_dict().items())
        for k, a in self.weights().items():
            sd[k] = torch.from_numpy(a).to(sd[k].dtype)
        return sd

    def publish(self):
        """The masters go into the model's own parameters, in place, and -- where the step has not put them there already --
        into the live context's inference forms: from here on validate_chunks, basecall_chunks and the model's forward
        compute with the trained layers."""
        trained = self.weights()
        own = self.model.state_dict(keep_vars=True)
        with torch.no_grad():
            for k, a in trained.items():
                own[k].copy_(torch.from_numpy(a))
        if self.reloads:
            # the live context, not Model.load_state_dict (which would drop it, and the trainer's state with it)
            self.ctx.load_state_dict({k: v.detach().to(torch.float32).cpu().numpy() for k, v in self.model.state_dict().items()})

    def close(self):
        """End the run: publish, then free the trainer's device state."""
        if self.ctx is None:
            return
        self.publish()
        self._end()
        self.ctx = None


class HeadTrainer(Trainer):
    # the step re-packs the head on the device: the live context already computes with the masters
    reloads = False

    def _keys(self):
        return [W_KEY, B_KEY]

    def _begin(self, arrays):
        self.ctx.head_train_begin(*arrays)

    def _step(self, sig, targets, lengths, lr):
        return self.ctx.head_train_step(sig, targets, lengths, lr)

    def _end(self):
        self.ctx.head_train_end()

    def _masters(self):
        return self.ctx.head_get_weights()


class TopTrainer(Trainer):

    def __init__(self, model, layers, chunk_len, batch):
        self.layers = int(layers)
        super().__init__(model, chunk_len, batch)

    def _keys(self):
        if not 1 <= self.layers <= 5:
            raise ValueError("%d unfrozen LSTM layers: 1 .. 5 can be trained (the convolutions stay frozen)" % self.layers)
        return top_keys(self.layers)

    def _begin(self, arrays):
        self.ctx.top_train_begin(self.layers, np.concatenate([a.ravel() for a in arrays]))

    def _step(self, sig, targets, lengths, lr):
        return self.ctx.top_train_step(sig, targets, lengths, lr)

    def _end(self):
        self.ctx.top_train_end()

    def grad(self, batch, targets, lengths):
        """The gradient of a (N,1,L) batch, left unclipped on the device -> (mean loss, gradient norm); no update."""
        return self.ctx.top_train_grad(self._signal(batch), targets, lengths)

    def _masters(self):
        sizes = [int(np.prod(shape)) for shape in self.shapes]
        return np.split(self.ctx.top_get_weights(), np.cumsum(sizes)[:-1])


class FullTrainer(TopTrainer):

    def __init__(self, model, chunk_len, batch):
        super().__init__(model, 5, chunk_len, batch)

    def _keys(self):
        keys = list(self.model.state_dict())
        if keys != full_keys():
            raise NotImplementedError("the trainer of every layer takes rnn_encoder's three convolutions, five LSTM layers and head; "
                                      "this model's state dict has other keys")
        return keys

    def _begin(self, arrays):
        self.ctx.full_train_begin(np.concatenate([a.ravel() for a in arrays]))
