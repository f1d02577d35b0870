#!/usr/bin/env python
"""GPU tool: two builds of libxnacall.so against each other, BYTE for byte -- scores (fp32), called sequences and lengths -- over
the shapes that exercise the recurrence's variants (one / two groups per workgroup, ragged groups, chunk slabs, small feature
sizes, every precision), each build loaded in its own process (XNA_LIBXNACALL).  Used in round 5 to show that the recurrence's
lean-issue rewrite (same arithmetic, fewer instructions) changes no bit:  python tools/lib_ab.py OLD.so NEW.so

TRAIN_CASES are the loss and training families on small contexts (chunks of 200 samples, at most 8): three steps each of a head
trainer, a top trainer at L = 1 and L = 2 and a full trainer with a validate_chunks between the first two, top_train_grad,
ctc_loss, ctc_loss_grad, validate_chunks, head_grad with and without X.  Their digests cover every returned float, the weights
after each step and the head's image.  --train runs these alone.

API_CASES are the inference calls on the same small contexts: decode with labels, decode_q and decode_ub in both layouts, crf_scans
with all four outputs, ctc_logz with gradients, ctc_alignments, beam_search, basecall_chunks_beam, basecall_chunks at the three
levels, two rounds of submit_chunks / collect_chunks over the four slots at each level, and one paired couple of
basecall_chunks_dev.  After each of them the digest takes every returned array and the `launches` of xb_get_stage_times: a call
launches exactly what it launched in the other build.  --api runs these alone."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [  # features, nb, chunk_len, n, precision, paired calls, env
    (768, 6, 2000, 512, "mixed", 2, {}),
    (768, 6, 1500, 512, "mixed", 1, {}),
    (768, 5, 1000, 1024, "mixed", 1, {}),
    (768, 6, 1000, 600, "f16f8", 1, {}),
    (768, 6, 1000, 513, "f16x3", 1, {}),
    (768, 6, 800, 1500, "mixed", 1, {}),
    (768, 5, 800, 200, "f16", 1, {}),
    (768, 6, 1000, 512, "mixed", 2, {"XB_OVERLAP": "0"}),
    (768, 6, 1000, 700, "mixed", 1, {"XB_LSTM_SPREAD": "1"}),
    (256, 6, 1000, 300, "mixed", 1, {}),
    (128, 5, 1000, 130, "f16f8", 1, {}),
    (96, 5, 1000, 70, "f16x3", 1, {}),
    (64, 6, 1000, 40, "mixed", 1, {}),
]
TRAIN_CASES = [(F, Lt) for F in (32, 64) for Lt in (12, 24)]       # features, label row width
API_CASES = [32, 64]                                               # features


def api_digest(F):
    import numpy as np
    import torch
    from xna_basecaller_amd import _lib
    from xna_basecaller_amd.synthetic import peaky_weights
    nb, sl, L, N, Lt, alphabet = 6, 3, 200, 8, 12, "NACGTXY"
    rng = np.random.default_rng(F)
    ctx = _lib.Context(0, nb, sl, F, 19, 5, 5.0, 2.0, L, N, precision=_lib.XB_PREC_MIXED)
    ctx.load_state_dict(peaky_weights(F, nb))
    h = hashlib.sha1()

    def add(out):
        """a case's arrays, then what the context has launched so far"""
        for a in (out.values() if isinstance(out, dict) else out):
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(np.array([v[1] for v in ctx.stage_times().values()], np.int64).tobytes())

    x = rng.standard_normal((N, L)).astype(np.float32)
    lens = rng.integers(sl, Lt + 1, N).astype(np.int32)
    targets = rng.integers(1, nb + 1, (N, Lt)).astype(np.int32)
    with_blank, without = ctx.encode(x, expand_blanks=True), ctx.encode(x, expand_blanks=False)
    add(ctx.decode(with_blank, alphabet, want_labels=True))
    add(ctx.decode(without, alphabet, want_labels=True))
    for sc in (with_blank, without):
        add(ctx.decode_q(sc, alphabet, 1.5, 0.25))
        add(ctx.decode_ub(sc, alphabet, 1.5, 0.25))
        add(ctx.beam_search(sc[:, :5], alphabet, beam_width=8))
    add(ctx.crf_scans(with_blank))
    add(ctx.ctc_logz(with_blank, targets, lens, want_grads=True))
    add(ctx.ctc_alignments(with_blank, targets, lens))
    add(ctx.basecall_chunks_beam(x[:5], alphabet, beam_width=8))
    for level in (0, 1, 2):
        add(ctx.basecall_chunks(x, alphabet, 1.5, 0.25, level=level))
    for level in (0, 1, 2):
        for _ in range(2):
            for slot in range(_lib.XB_PIPELINE_SLOTS):
                ctx.submit_chunks(slot, x[slot:], alphabet, 1.5, 0.25, level=level)
            for slot in range(_lib.XB_PIPELINE_SLOTS):
                add(ctx.collect_chunks(slot, N - slot, level=level))
    ctx.reserve_pairing()
    dx = torch.from_numpy(x).cuda()
    bufs = [(torch.zeros((n, ctx.T), dtype=torch.int8, device="cuda"), torch.zeros((n,), dtype=torch.int32, device="cuda")) for n in (N, 3)]
    for s, l in bufs:
        ctx.basecall_chunks_dev(dx.data_ptr(), s.shape[0], alphabet, s.data_ptr(), l.data_ptr())
    ctx.synchronize()
    add([a.cpu().numpy() for pair in bufs for a in pair])
    ctx.close()
    return h.hexdigest()


def train_digest(F, Lt):
    import numpy as np
    from xna_basecaller_amd import _lib
    from xna_basecaller_amd.crf.trainer import B_KEY, W_KEY, full_keys, top_keys
    from xna_basecaller_amd.synthetic import seeded_weights
    nb, sl, L, N, alphabet = 6, 3, 200, 8, "NACGTXY"
    sd = seeded_weights(F, nb)
    rng = np.random.default_rng(F + Lt)
    h = hashlib.sha1()

    def add(*arrays):
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())

    def batch(n):
        lens = rng.integers(sl, Lt + 1, n).astype(np.int32)
        targets = np.zeros((n, Lt), np.uint8)
        for i in range(n):
            targets[i, :lens[i]] = rng.integers(1, nb + 1, lens[i])
        return rng.standard_normal((n, L)).astype(np.float32), targets, lens

    def context():
        ctx = _lib.Context(0, nb, sl, F, 19, 5, 5.0, 2.0, L, N, precision=_lib.XB_PREC_MIXED)
        ctx.load_state_dict(sd)
        return ctx

    flat = lambda keys: np.concatenate([sd[k].ravel() for k in keys])                          # noqa: E731
    batches = [batch(n) for n in (8, 3, 8)]
    for kind in ("head", 1, 2, "full"):
        ctx = context()
        if kind == "head":
            ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
        elif kind == "full":
            ctx.full_train_begin(flat(full_keys()))
        else:
            ctx.top_train_begin(kind, flat(top_keys(kind)))
        for i, (x, t, l) in enumerate(batches):
            if kind == "head":
                add(np.array(ctx.head_train_step(x, t, l, 2e-3), np.float32), *ctx.head_get_weights())
                add(*ctx.head_image())
            else:
                add(np.array(ctx.top_train_step(x, t, l, 2e-3), np.float32), ctx.top_get_weights())
            if i == 0:
                add(*ctx.validate_chunks(x, alphabet, t, l))
        if kind == "head":
            ctx.head_train_end()
        else:
            add(np.array(ctx.top_train_grad(*batches[1]), np.float32))
            ctx.top_train_end()
        ctx.close()

    ctx = context()
    x, t, l = batches[0]
    y = ctx.encode(x, expand_blanks=False)
    for sc in (y, ctx.encode(x, expand_blanks=True)):
        add(*ctx.ctc_loss(sc, t, l, has_blank=None if sc is y else True, want_logz=True))
        add(*ctx.ctc_loss_grad(sc, t, l))
    add(*ctx.validate_chunks(x, alphabet, t, l))
    loss, dy = ctx.ctc_loss_grad(y, t, l)
    ctx.encode(x, expand_blanks=False)                          # X = None: the last encoder pass
    add(*ctx.head_grad(y, dy))
    M = y.shape[0] * y.shape[1]
    x_hi = rng.standard_normal((M, F)).astype(np.float16)
    x_lo = (rng.standard_normal((M, F)) * 2.0 ** -11).astype(np.float16)
    add(*ctx.head_grad(y, dy, x_hi.view(np.uint16), x_lo.view(np.uint16)))
    ctx.close()
    return h.hexdigest()


def worker(only=None):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from xna_basecaller_amd import _lib
    from xna_basecaller_amd.synthetic import peaky_weights, seeded_weights
    out = []
    for F, nb, L, n, prec, calls, env in ([] if only else CASES):
        os.environ.update(env)
        ctx = _lib.Context(0, nb, 3, F, 19, 5, 5.0, 2.0, L, n, precision=_lib.PRECISIONS[prec])
        for k in env:
            os.environ.pop(k)
        ctx.load_state_dict(peaky_weights(F, nb) if F == 768 else seeded_weights(F, nb))
        if calls > 1:
            ctx.reserve_pairing()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(F + n)
        xs = [torch.randn((n, L), dtype=torch.float32, device="cuda", generator=gen) for _ in range(calls)]
        alphabet = "NACGTXY"[:nb + 1]
        bufs = [(torch.empty((n, ctx.T), dtype=torch.int8, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda")) for _ in xs]
        for x, (s, l) in zip(xs, bufs):
            ctx.basecall_chunks_dev(x.data_ptr(), n, alphabet, s.data_ptr(), l.data_ptr())
        ctx.synchronize()
        h = hashlib.sha1()
        for s, l in bufs:
            h.update(s.cpu().numpy().tobytes())
            h.update(l.cpu().numpy().tobytes())
        scores = ctx.encode(xs[0].cpu().numpy())
        h.update(np.ascontiguousarray(scores).tobytes())
        out.append(h.hexdigest())
        ctx.close()
    out += [train_digest(F, Lt) for F, Lt in TRAIN_CASES] if only != "--api" else []
    out += [api_digest(F) for F in API_CASES] if only != "--train" else []
    print("DIGESTS " + json.dumps(out))


def main():
    only = ([a for a in sys.argv[1:] if a in ("--train", "--api")] or [None])[0]
    argv = [a for a in sys.argv[1:] if a != only]
    if argv == ["--worker"]:
        return worker(only)
    libs = argv[:2]
    cases = [] if only else list(CASES)
    cases += [("train", "features %d" % F, "label rows %d wide" % Lt) for F, Lt in TRAIN_CASES] if only != "--api" else []
    cases += [("api", "features %d" % F) for F in API_CASES] if only != "--train" else []
    res = []
    for lib in libs:
        env = dict(os.environ, XNA_LIBXNACALL=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + [only] * bool(only), env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        line = [l for l in r.stdout.decode().splitlines() if l.startswith("DIGESTS ")]
        if r.returncode or not line:
            print(r.stderr.decode()[-2000:])
            print("lib_ab: %s failed (rc %d)" % (lib, r.returncode))
            return 1
        res.append(json.loads(line[0][8:]))
    bad = 0
    for case, a, b in zip(cases, res[0], res[1]):
        same = a == b
        bad += not same
        print("%-60s %s" % (str(case), "identical" if same else "DIFFERENT  %s vs %s" % (a[:10], b[:10])))
    print("lib_ab:", "OK -- every byte identical" if not bad else "%d cases differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
