"""MBR step: the native formulation (pika_amd/mbr.py: device trajectories, split
joint, sparse risk surrogate) against a literal restatement of the reference's inline code
(train_transducer_mbr_bmuf_otfaug.py:169-235: dense one-hot gradient, concatenated joint input,
Python trajectory loops) on the same model, N-best lists and scores."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_common as C  # noqa: E402
import decode_common as D  # noqa: E402
from test_decode import build  # noqa: E402


def reference_mbr(model, x_feats, target, ali_lens, hyps, scores, beam, blk, sm_scale, pad):
    """Lines :124-138 (encoder) and :163-235, restated with the reference's tensor ops."""
    import editdistance
    x = model.encoder(x_feats)
    T = x.size(1)
    bsz = x.size(0)
    bb = bsz * beam
    x = x.unsqueeze(1).expand(-1, beam, -1, -1).contiguous().view(bb, -1, model.hid_dim)
    prob = F.softmax(torch.tensor([[float(s) for s in r] for r in scores]).view(bsz, beam).to(x.device), dim=1)
    dist = torch.zeros(bsz, beam, device=x.device)
    nb, maxl = [], 0
    for i in range(bsz):
        nb.append([[int(e) for e in hyps[i][j] if int(e) != blk] for j in range(beam)])
        maxl = max(maxl, max(len(h) for h in nb[i]))
    U = maxl + 1
    for i in range(bsz):
        ref = target[i][:ali_lens[i]].tolist()
        for j in range(beam):
            dist[i][j] = editdistance.eval(ref, nb[i][j])
            nb[i][j] = nb[i][j] + (maxl - len(nb[i][j])) * [pad]
    avg = (prob * dist).sum(dim=1)
    mbr_loss = avg.sum()
    seq_grad = prob * (dist - avg.unsqueeze(1))
    y = torch.tensor(nb, device=x.device).view(bb, -1)
    y = torch.cat((torch.zeros(bb, 1, dtype=torch.long, device=x.device), y), dim=1)
    y = model.predict(y)
    b_idx, x_idx, y_idx = [], [], []
    mbr_grad = x.new_zeros(bb, T + U, model.output_dim)
    for i in range(bsz):
        for j in range(beam):
            h = [int(e) for e in hyps[i][j]]
            t_idx, u_idx = [0], [0]
            for t in range(1, len(h)):
                t_idx.append(t_idx[t - 1] + int(h[t - 1] == blk))
                u_idx.append(u_idx[t - 1] + int(h[t - 1] != blk))
            t_idx.extend((T + U - len(t_idx)) * [0]); u_idx.extend((T + U - len(u_idx)) * [0])
            x_idx.extend(t_idx); y_idx.extend(u_idx); b_idx.extend([i * beam + j] * (T + U))
            if h:
                mbr_grad[i * beam + j, torch.arange(len(h)), h] = seq_grad[i][j]
    joint = torch.cat((x[b_idx, x_idx, :], y[b_idx, y_idx, :]), dim=-1).view(bb, T + U, -1)
    out = model.fc2(torch.tanh(model.fc1(joint)) * torch.sigmoid(model.fc_gate(joint)))
    out = F.log_softmax(sm_scale * out, dim=-1)
    mbr_grad[:, :, blk] = mbr_grad[:, :, blk] / float(T)
    out.backward(mbr_grad)
    return float(mbr_loss), seq_grad.detach()


def run(device):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pika_amd", "dropin"))
    from decoder.transducer_decoder import TransducerDecoder
    from decoder.beam_transducer import GlobalScorer
    from pika_amd import mbr
    net = build("transformer", device)
    x, y, y_len, _ = [t.to(device) for t in C.inputs()]
    _, x_len = D.inputs()
    beam, blk, sm = 3, 0, 0.9
    args = SimpleNamespace(las_rescorer=None, las_rescorer_bw=None, bilas_rescorer=None, nonblk_reward=0.0)
    net.eval()
    dec = TransducerDecoder(net, 4, beam, n_best=beam, blk=blk, global_scorer=GlobalScorer(), sm_scale=sm,
                            cuda=(device != "cpu"), args=args)
    ret, _ = dec.decode_batch(x, x_len.to(device), [int(a) + int(b) + 3 for a, b in zip(x_len, y_len)])  # :114
    hyps, scores = ret["predictions"], ret["scores"]
    assert any(0 < sum(1 for e in h if int(e) != blk) for row in hyps for h in row)
    net.train()
    # reference formulation
    net.zero_grad()
    loss_ref, sg_ref = reference_mbr(net, x, y, y_len, hyps, scores, beam, blk, sm, C.V)
    g_ref = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    # native formulation
    net.zero_grad()
    enc = net.encoder(x)
    prob, dist, seq_grad, nonblk = mbr.risk_terms(hyps, scores, y, y_len, blk, enc.device)
    assert torch.allclose(seq_grad, sg_ref, atol=1e-6)
    assert abs(float((prob * dist).sum()) - loss_ref) < 1e-4
    mbr.mbr_backward(net, enc, hyps, seq_grad, nonblk, blk, sm)
    for k, p in net.named_parameters():
        if k in g_ref:
            scale = g_ref[k].abs().max().item()
            err = (p.grad - g_ref[k]).abs().max().item()
            assert err <= 2e-3 * scale + 1e-6, (k, err, scale)
    assert set(g_ref) == {k for k, p in net.named_parameters() if p.grad is not None}


def test_cpu_native_mbr_equals_reference_formulation():
    run("cpu")


@pytest.mark.gpu
def test_gpu_native_mbr_equals_reference_formulation(hip_device):
    from pika_amd import gemm as G
    old, G.PRECISION = G.PRECISION, "fp32"
    try:
        run(hip_device)
    finally:
        G.PRECISION = old


@pytest.mark.gpu
def test_risk_grad_kernel(hip_device):
    from pika_amd.mbr import RiskFn
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(37, 100, generator=g, dtype=torch.float64)
    sym = torch.randint(0, 100, (37,), generator=g)
    val = torch.randn(37, generator=g, dtype=torch.float64)
    val[5] = 0.0
    lr = logits.clone().requires_grad_(True)
    (F.log_softmax(0.8 * lr, -1).gather(1, sym.unsqueeze(1)).squeeze(1) * val).sum().backward()
    ld = logits.float().to(hip_device).requires_grad_(True)
    s = RiskFn.apply(ld * 1.0, sym.int().to(hip_device), val.float().to(hip_device), 0.8)
    s.backward()
    assert (ld.grad.double().cpu() - lr.grad).abs().max() < 1e-5
    assert torch.all(ld.grad[5] == 0)


# ---- pinned against the reference SCRIPT itself (tests/golden/make_mbr_script_golden.py) ---------------------------
GOLD_SCRIPT = os.path.join(HERE, "golden", "mbr_script_grads.npz")
MBR_SCRIPT = "/root/reference/trainer/train_transducer_mbr_bmuf_otfaug.py"


@pytest.mark.skipif(not os.path.exists(MBR_SCRIPT), reason="reference tree not present on this box")
def test_unchanged_mbr_script_on_the_dropins_reproduces_the_reference_gradients(tmp_path):
    """The UNCHANGED train_transducer_mbr_bmuf_otfaug.py, one batch, every parameter gradient before its first
    optimizer step: run on the drop-in packages (CPU tensors) vs the golden recorded from the same script on the
    reference's own trainer.model.* / decoder.* -- same N-best, gradients to 1e-3."""
    import subprocess
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import mbr_hooks as M
    from bmuf_common import free_port
    out = str(tmp_path / "dropin.npz")
    env = dict(os.environ, MASTER_PORT=str(free_port()), OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "mbr_hooks.py"), "dropin", out], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got, want = np.load(out), np.load(GOLD_SCRIPT)
    assert np.array_equal(got["hyps"], want["hyps"])
    assert np.abs(got["scores"] - want["scores"]).max() < 1e-4
    M.compare(got, want, rel=1e-3)


def _native_step_vs_script_golden(device, search_precision=None, _raw=False, graphed=False):
    """pika_amd.mbr (device trajectories, split joint, sparse risk surrogate / HIP risk-gradient kernel) fed with
    the same seeded model and fixture batch as the golden run of the reference script: same N-best out of the
    drop-in decoder, and RNN-T + risk gradients equal to what the script's inline code produced."""
    import argparse
    sys.path.insert(0, os.path.join(HERE, "golden"))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pika_amd", "dropin"))
    import importlib.util
    import mbr_hooks as M
    spec = importlib.util.spec_from_file_location(
        "mbr_fixture_loader", os.path.join(HERE, "golden", "mbr_fixture", "loader", "otf_utt_loader.py"))
    fixture = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fixture)
    from oracle.pika_ref import seeded_state_dict
    from model.transducer import Net
    from decoder.transducer_decoder import TransducerDecoder
    from decoder.beam_transducer import GlobalScorer
    from pika_amd import mbr
    from pika_amd.model import ops
    want = np.load(GOLD_SCRIPT)
    ap = argparse.ArgumentParser()
    for k in ("--encoder_type", "--decoder_type", "--rnn_type"):
        ap.add_argument(k)
    for k in ("--enc_layers", "--dec_layers", "--rnn_size", "--embd_dim", "--padding_idx", "--output_dim"):
        ap.add_argument(k, type=int)
    ap.add_argument("--dropout", type=float)
    opt = ap.parse_args(M.MODEL_ARGS)
    opt.local_rank, opt.brnn = 0, False
    net = Net(opt, 240, M.V)
    net.encoder = type(net.encoder)(240, 0, opt.rnn_size, tdnn_nhid=64, tdnn_layers=6)
    net.pack_seq = False
    sd = seeded_state_dict(net, 1234)
    sd["fc2.bias"][0] += 1.5
    net.load_state_dict(sd)
    net = net.to(device)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    largs = SimpleNamespace(feats_dim=80, lctx=1, rctx=1, batch_size=3, fixture_seed=31, fixture_batches=1,
                            output_dim=M.V, padding_idx=M.V)
    data, target, lens, ali = next(iter(fixture.dataloader(None, None, None, largs)))
    data, target, ali = data.to(device), target.long().to(device), ali.to(device)
    len_b = lens.to(device) - 24
    len_b = len_b // 4 + (len_b % 4 != 0).int()
    beam, blk, sm, rnnt_scale = 3, 0, 0.9, 0.1
    dargs = SimpleNamespace(las_rescorer=None, las_rescorer_bw=None, bilas_rescorer=None, nonblk_reward=0.0)
    net.eval()
    dec = TransducerDecoder(net, 3, beam, n_best=beam, blk=blk, global_scorer=GlobalScorer(), sm_scale=sm,
                            cuda=(device != "cpu"), beam_prune=False, args=dargs)
    if search_precision is not None:
        dec.decode_precision = search_precision
    ret, _ = dec.decode_batch(data, len_b, len_b + ali + 3)                         # :112-117
    hyps, scores = ret["predictions"], ret["scores"]
    L = want["hyps"].shape[2]
    got_h = np.full(want["hyps"].shape, -1, np.int64)
    for b, row in enumerate(hyps):
        for j, h in enumerate(row):
            got_h[b, j, :len(h)] = [int(e) for e in h]
    score_err = np.abs(np.array([[float(v) for v in r] for r in scores]) - want["scores"]).max()
    if search_precision == "bf16":
        # one bf16 term per operand carries no parity claim (8-bit mantissas: near-ties between deep entries trade places with
        # any change of the product order, e.g. linear_out folded into the joint's prediction halves): the top-1 hypotheses
        # are asserted, the rest is reported
        assert np.array_equal(got_h[:, 0], want["hyps"][:, 0])
        same = int((got_h == want["hyps"]).all(axis=2).sum())
        # bounded, not free: most entries at the reference rank (measured 7 of 9), and whatever moved is the SAME
        # set of hypotheses per utterance in another order, with scores within the one-term noise
        n_all = got_h.shape[0] * got_h.shape[1]
        assert same >= (6 * n_all + 8) // 9, (same, n_all)
        for b in range(got_h.shape[0]):
            assert sorted(map(tuple, got_h[b].tolist())) == sorted(map(tuple, want["hyps"][b].tolist())), b
        assert score_err < 0.1, score_err
        print("bf16 N-best search: top-1 identical, %d of %d entries at the reference rank, max |score diff| %.2e"
              % (same, got_h.shape[0] * got_h.shape[1], score_err))
        if _raw is False:
            return None, None, None
    else:
        assert np.array_equal(got_h, want["hyps"])
        assert score_err < 2e-3, score_err
    net.train()
    net.zero_grad()
    if graphed:
        # the training half as ONE hipGraph (pika_amd.mbr.GraphedMbrStep): an eager warm-up call, the capture, two replays;
        # dropout is off, so every call leaves the same gradients -- the LAST replay's are compared
        step = mbr.GraphedMbrStep(net, rnnt_scale=rnnt_scale, sm_scale=sm, blk=blk, min_seen=1, warmup=1)
        for _ in range(4):
            net.zero_grad(set_to_none=True)
            step(data, target, len_b.int(), ali.int(), hyps, scores)
        assert step.broken is None, step.broken
        assert step.stats == {"replays": 3, "captures": 1, "eager": 1, "evictions": 0}, step.stats
        grads = {"g%03d" % i: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy()
                 for i, p in enumerate(net.parameters())}
        step.close()
        if _raw == "names":
            return M, dict(M.compact(grads), n=np.array(len(grads)), names=[k for k, _ in net.named_parameters()]), want
        return M, dict(M.compact(grads), n=np.array(len(grads))), want
    enc = net.encoder(data)                                                       # :124-138
    sos = torch.zeros(3, 1, dtype=torch.long, device=device)
    pred = net.predict(torch.cat((sos, target), dim=1))
    lp = ops.joint(enc, pred, net.fc1, net.fc_gate, net.fc2, log_softmax=True)
    if device == "cpu":
        from oracle import rnnt as O
        costs, g = O.rnnt_loss(lp.detach().numpy(), target.int().numpy(), len_b.int().numpy(), ali.int().numpy(),
                               dtype=np.float32)
        lp.backward(rnnt_scale * torch.from_numpy(g), retain_graph=True)          # the checker stands in on CPU
    else:
        from pika_amd.rnnt import RNNTLoss
        (rnnt_scale * RNNTLoss(blank=0).apply(lp, target.int(), len_b.int(), ali.int())).sum().backward(retain_graph=True)
    part = os.environ.get("PIKA_MBR_DEBUG_PART", "both") if _raw is True else "both"      # tools/mbr_mode_diff.py
    if part == "risk":
        net.zero_grad()
    if part != "rnnt":
        prob, dist, seq_grad, nonblk = mbr.risk_terms(hyps, scores, target, ali, blk, enc.device)
        mbr.mbr_backward(net, enc, hyps, seq_grad, nonblk, blk, sm)
    grads = {"g%03d" % i: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy()
             for i, p in enumerate(net.parameters())}
    if _raw == "names":
        return M, dict(M.compact(grads), n=np.array(len(grads)), names=[k for k, _ in net.named_parameters()]), want
    if _raw:
        return M, {"names": [k for k, _ in net.named_parameters()], "grads": list(grads.values())}, want
    got = dict(M.compact(grads), n=np.array(len(grads)))
    return M, got, want


def test_cpu_native_mbr_step_matches_the_reference_script_golden():
    M, got, want = _native_step_vs_script_golden("cpu")
    M.compare(got, want, rel=1e-3)


@pytest.mark.gpu
def test_gpu_native_mbr_step_matches_the_reference_script_golden(hip_device):
    from pika_amd import gemm as G
    old, G.PRECISION = G.PRECISION, "fp32"
    try:
        M, got, want = _native_step_vs_script_golden(hip_device)
    finally:
        G.PRECISION = old
    M.compare(got, want, rel=2e-3)


@pytest.mark.gpu
def test_gpu_graphed_mbr_training_half_matches_the_reference_script_golden(hip_device):
    """The training half of the step as ONE replayed hipGraph (GraphedMbrStep: one backward pass over rnnt + surrogate
    instead of the script's two) in the exact arithmetic: the gradients the unchanged reference script left in .grad
    (train_transducer_mbr_bmuf_otfaug.py:120-235), to the same 2e-3 as the eager native step."""
    from pika_amd import gemm as G
    old, G.PRECISION = G.PRECISION, "fp32"
    try:
        M, got, want = _native_step_vs_script_golden(hip_device, graphed=True)
    finally:
        G.PRECISION = old
    M.compare(got, want, rel=2e-3)


def _worst(got, want, names):
    """(worst sample error, worst L2-norm difference) over the parameters of two compact dumps, each relative to the
    parameter's gradient scale: its own max |g| -- or, for a bias, its weight's if that is larger.  A bias whose gradient
    is mathematically ZERO (the key projection's: softmax is invariant to a constant added to every score of a query; a
    bias in front of BatchNorm) holds only rounding noise in any arithmetic (exact mode: 3e-8 on this fixture; bf16
    backward products: 1.5e-3, i.e. 1.5 % of the key WEIGHT's gradient), so its own scale says nothing."""
    scale = {}
    for i, n in enumerate(names):
        scale[n] = float(want["m%03d" % i][2])
    ws, wn, who = 0.0, 0.0, None
    for i, n in enumerate(names):
        k = "%03d" % i
        ms, mg = want["m" + k], got["m" + k]
        sc = max(scale[n], scale.get(n[:-4] + "weight", 0.0) if n.endswith(".bias") else 0.0)
        if sc < 1e-12:
            continue
        e = float(np.abs(got["s" + k] - want["s" + k]).max() / sc)
        if e > ws:
            ws, who = e, n
        wn = max(wn, float(abs(mg[0] - ms[0]) / (ms[0] * sc / scale[n])) if scale[n] > 0 else 0.0)
    return ws, wn, who


@pytest.mark.gpu
def test_gpu_native_mbr_step_in_the_benchmarked_arithmetic(hip_device):
    """The same step in the arithmetic bench.py's MBR leg runs: the PACKAGE-DEFAULT product mode ("mixed": two-term
    forward, bf16 backward) with the N-best search in the default decode arithmetic (two fp16 terms) -- against the
    golden of the unchanged reference script.  The N-best (hypotheses, blanks included) must be the script's, scores
    within 2e-3.  Gradients carry the bf16 rounding of every backward product (2^-9 per operand): measured on MI355X,
    8e-2 of the parameter's largest entry on the prediction net's query / key projections (softmax backward: d(scores)
    rows sum to zero, so their bf16 rounding is a relative error of the small remainder), <= 2e-2 elsewhere; held to
    0.15 / 0.15 (the printed line has the measured values and the worst parameter).  The one-term bf16 search is run as
    well: on this fixture it must return the same N-best (NOT what bench.py times)."""
    from pika_amd import gemm as G
    assert G.PRECISION == "mixed"
    M, got, want = _native_step_vs_script_golden(hip_device, _raw="names")
    ws, wn, who = _worst(got, want, got["names"])
    print("MBR step, default arithmetic: N-best identical; worst gradient sample error %.2e of the parameter's scale "
          "(%s), worst parameter-norm difference %.2e" % (ws, who, wn))
    assert ws < 0.15 and wn < 0.15, (ws, wn, who)
    _native_step_vs_script_golden(hip_device, search_precision="bf16")   # asserts the N-best inside
    # ... and as bench.py's MBR leg runs the training half: ONE replayed hipGraph (pika_amd.mbr.GraphedMbrStep)
    M, got, want = _native_step_vs_script_golden(hip_device, _raw="names", graphed=True)
    ws, wn, who = _worst(got, want, got["names"])
    print("MBR step, default arithmetic, graphed training half: worst gradient sample error %.2e of the parameter's scale "
          "(%s), worst parameter-norm difference %.2e" % (ws, who, wn))
    assert ws < 0.15 and wn < 0.15, (ws, wn, who)


def test_edit_distances_library_call_equals_the_python_dp():
    """pika_edit_distances (host code of libpika_amd.so, all N-best pairs of a batch in one call) against the plain
    dynamic programme and hand cases -- what editdistance.eval returns (requirements.txt:1 of the reference)."""
    import random
    from pika_amd import mbr
    assert mbr.edit_distances([([1, 2, 3], [1, 2, 3]), ([], [4, 5]), ([7], []), ([1, 2, 3, 4], [2, 3, 5]), ([], [])]) == \
        [0, 2, 1, 2, 0]
    random.seed(3)
    pairs = [([random.randrange(6) for _ in range(random.randrange(0, 40))],
              [random.randrange(6) for _ in range(random.randrange(0, 25))]) for _ in range(200)]
    assert mbr.edit_distances(pairs) == [mbr.edit_distance(a, b) for a, b in pairs]
    assert mbr.edit_distances([]) == []


def _edit_distances_abi(seqs, a_off, a_len, b_off, b_len, n_pairs=None):
    """pika_edit_distances itself (pika_amd.mbr.edit_distances returns early on an empty list): (rc, out)."""
    from pika_amd import _lib
    n = len(a_len) if n_pairs is None else n_pairs
    seqs = np.asarray(list(seqs) + [-99], dtype=np.int32)               # never empty, and a guard nobody may compare
    ao, bo = np.asarray(list(a_off) + [0], dtype=np.int64), np.asarray(list(b_off) + [0], dtype=np.int64)
    al, bl = np.asarray(list(a_len) + [0], dtype=np.int32), np.asarray(list(b_len) + [0], dtype=np.int32)
    out = np.full(len(a_len) + 1, -7, dtype=np.int32)
    rc = _lib.lib().pika_edit_distances(seqs.ctypes.data, ao.ctypes.data, al.ctypes.data, bo.ctypes.data, bl.ctypes.data,
                                        n, out.ctypes.data)
    return rc, out.tolist()


def test_edit_distances_edge_cases_at_the_abi():
    """n_pairs == 0 writes nothing; two empty sequences are 0 apart; an empty one against n symbols is n (either side);
    identical sequences are 0 apart (also one sequence against itself at the same offset); a negative length in ANY pair is
    PIKA_EINVAL and nothing is written."""
    assert _edit_distances_abi([], [], [], [], []) == (0, [-7])
    assert _edit_distances_abi([1, 2, 3], [0], [3], [0], [3], n_pairs=0) == (0, [-7, -7])
    assert _edit_distances_abi([], [0], [0], [0], [0]) == (0, [0, -7])
    assert _edit_distances_abi([5, 6, 7], [0], [0], [0], [3]) == (0, [3, -7])
    assert _edit_distances_abi([5, 6, 7], [0], [3], [3], [0]) == (0, [3, -7])
    assert _edit_distances_abi([4, 4, 9, 4, 4, 9], [0], [3], [3], [3]) == (0, [0, -7])
    assert _edit_distances_abi([4, 4, 9], [0], [3], [0], [3]) == (0, [0, -7])
    # several pairs in one call, an empty one between two others: the rolling rows are sized by the longest b
    assert _edit_distances_abi([1, 2, 3, 1, 9, 3, 8], [0, 0, 3], [3, 0, 3], [3, 0, 6], [3, 0, 1]) == (0, [1, 0, 3, -7])
    for a_len, b_len in (([-1], [2]), ([2], [-1]), ([2, -3], [2, 2]), ([2, 2], [2, -1])):
        off = [0] * len(a_len)
        rc, out = _edit_distances_abi([1, 2, 3, 4], off, a_len, off, b_len)
        assert rc == -1 and out == [-7] * (len(a_len) + 1), (a_len, b_len)
    assert _edit_distances_abi([1, 2], [0], [1], [1], [1], n_pairs=-1)[0] == -1


@pytest.mark.gpu
def test_gpu_graphed_mbr_step_replays_on_other_nbest_lists_and_buckets(hip_device):
    """GraphedMbrStep beyond the fixed batch of the golden: ONE captured graph must serve other N-best lists of its (S, U)
    bucket -- other symbols, lengths, scores, targets: everything travels through the static inputs -- a list outside the
    bucket gets its own graph, and every call leaves the gradients of the eager step (the script's two backward passes,
    `eager_step`) on the same weights.  Exact arithmetic; dropout off."""
    import copy
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pika_amd", "dropin"))
    from types import SimpleNamespace as NS
    from oracle.pika_ref import seeded_state_dict
    from model.transducer import Net
    from pika_amd import gemm as G
    from pika_amd import mbr
    V, B, beam, T_in, U = 120, 3, 3, 150, 6
    opt = NS(rnn_size=64, local_rank=0, decoder_type="transformer", brnn=False, encoder_type="tdnn", dropout=0.0,
             enc_layers=2, dec_layers=1, embd_dim=32, padding_idx=V)
    net = Net(opt, 240, V)
    net.encoder = type(net.encoder)(240, 0, 64, tdnn_nhid=64, tdnn_layers=6)
    net.pack_seq = False
    net.load_state_dict(seeded_state_dict(net, 77))
    net = net.to(hip_device).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    g = torch.Generator().manual_seed(5)
    Tp = (T_in - 24 + 3) // 4
    old, G.PRECISION = G.PRECISION, "fp32"
    step = mbr.GraphedMbrStep(net, rnnt_scale=0.1, sm_scale=0.9, blk=0, min_seen=1, warmup=1, s_bucket=32, u_bucket=8)
    ref_step = mbr.GraphedMbrStep(copy.deepcopy(net), rnnt_scale=0.1, sm_scale=0.9, blk=0)

    def batch(n_lab, seed):
        gg = torch.Generator().manual_seed(seed)
        feats = torch.randn(B, T_in, 240, generator=gg).to(hip_device)
        labels = torch.randint(1, V, (B, U), generator=gg)
        ali = torch.tensor([U, U - 1, U - 2], dtype=torch.int32)
        for b in range(B):
            labels[b, int(ali[b]):] = V
        x_len = torch.full((B,), Tp, dtype=torch.int32)
        hyps, scores = [], []
        for b in range(B):
            row, sc = [], []
            for j in range(beam):
                nl = max(1, n_lab - j - b)                      # labels of this hypothesis
                nb = Tp - int(torch.randint(0, 3, (1,), generator=gg))
                sym = [0] * nb + [int(v) for v in torch.randint(1, V, (nl,), generator=gg)]
                perm = torch.randperm(len(sym), generator=gg).tolist()
                row.append([torch.tensor(sym[i]) for i in perm])
                sc.append(torch.tensor(-1.0 - 0.3 * j - 0.01 * float(torch.rand(1, generator=gg))))
            hyps.append(row)
            scores.append(sc)
        return feats, labels.to(hip_device), x_len.to(hip_device), ali.to(hip_device), hyps, scores

    def grads_of(fn, args):
        fn.model.zero_grad(set_to_none=True)
        out = fn(*args) if fn is step else fn.eager_step(*args)
        torch.cuda.synchronize()
        return float(out), [None if p.grad is None else p.grad.detach().clone() for p in fn.model.parameters()]
    try:
        # same bucket three times (S = Tp + ~5..8 -> 64; U <= 8), then a longer label count (U bucket 16): a second graph
        for n_lab, seed in ((5, 1), (7, 2), (4, 3), (12, 4), (6, 5)):
            args = batch(n_lab, seed)
            got_loss, got = grads_of(step, args)
            want_loss, want = grads_of(ref_step, args)
            assert abs(got_loss - want_loss) <= 1e-4 * abs(want_loss) + 1e-5, (n_lab, got_loss, want_loss)
            for (name, _), a, b in zip(net.named_parameters(), got, want):
                if b is None:
                    assert a is None or float(a.abs().max()) == 0.0, name
                    continue
                scale = float(b.abs().max()) + 1e-12
                assert a is not None and float((a - b).abs().max()) <= 2e-3 * scale + 1e-7, (n_lab, name, float((a - b).abs().max()), scale)
        assert step.broken is None, step.broken
        # call 1 eager (warm-up), call 2 captures the first bucket, 3 replays it, 4 captures the wider label bucket, 5 is back on the first
        assert step.stats["captures"] == 2 and step.stats["replays"] == 4 and step.stats["eager"] == 1, step.stats
        assert len(step.entries) == 2
    finally:
        G.PRECISION = old
        step.close()


@pytest.mark.gpu
def test_gpu_graphed_mbr_step_on_batches_whose_shapes_never_recur(hip_device):
    """A corpus whose frame and label counts differ from batch to batch: no exact shape repeats, so a bucket of 64 frames x 8
    labels that has shown two shapes gets a graph at its upper boundary (192 frames, 8 labels) which the later batches of
    the bucket ride -- padding frames masked, labels padded -- and every call leaves the gradients of the eager step
    (`eager_step`) on the same weights.  Exact arithmetic; dropout off."""
    import copy
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pika_amd", "dropin"))
    from types import SimpleNamespace as NS
    from oracle.pika_ref import seeded_state_dict
    from model.transducer import Net
    from pika_amd import gemm as G
    from pika_amd import mbr
    V, B, beam, T_in, U = 120, 3, 3, 150, 6
    opt = NS(rnn_size=64, local_rank=0, decoder_type="transformer", brnn=False, encoder_type="tdnn", dropout=0.0,
             enc_layers=2, dec_layers=1, embd_dim=32, padding_idx=V)
    net = Net(opt, 240, V)
    net.encoder = type(net.encoder)(240, 0, 64, tdnn_nhid=64, tdnn_layers=6)
    net.pack_seq = False
    net.load_state_dict(seeded_state_dict(net, 77))
    net = net.to(hip_device).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    g = torch.Generator().manual_seed(5)
    old, G.PRECISION = G.PRECISION, "fp32"
    step = mbr.GraphedMbrStep(net, rnnt_scale=0.1, sm_scale=0.9, blk=0, min_seen=2, warmup=1, s_bucket=64, u_bucket=16)
    ref_step = mbr.GraphedMbrStep(copy.deepcopy(net), rnnt_scale=0.1, sm_scale=0.9, blk=0)

    def batch(n_lab, seed, T_in, U):
        Tp = (T_in - 24 + 3) // 4
        gg = torch.Generator().manual_seed(seed)
        feats = torch.randn(B, T_in, 240, generator=gg).to(hip_device)
        labels = torch.randint(1, V, (B, U), generator=gg)
        ali = torch.tensor([U, U - 1, max(U - 2, 1)], dtype=torch.int32)
        for b in range(B):
            labels[b, int(ali[b]):] = V
        x_len = torch.full((B,), Tp, dtype=torch.int32)
        hyps, scores = [], []
        for b in range(B):
            row, sc = [], []
            for j in range(beam):
                nl = max(1, n_lab - j - b)                      # labels of this hypothesis
                nb = Tp - int(torch.randint(0, 3, (1,), generator=gg))
                sym = [0] * nb + [int(v) for v in torch.randint(1, V, (nl,), generator=gg)]
                perm = torch.randperm(len(sym), generator=gg).tolist()
                row.append([torch.tensor(sym[i]) for i in perm])
                sc.append(torch.tensor(-1.0 - 0.3 * j - 0.01 * float(torch.rand(1, generator=gg))))
            hyps.append(row)
            scores.append(sc)
        return feats, labels.to(hip_device), x_len.to(hip_device), ali.to(hip_device), hyps, scores

    def grads_of(fn, args):
        fn.model.zero_grad(set_to_none=True)
        out = fn(*args) if fn is step else fn.eager_step(*args)
        torch.cuda.synchronize()
        return float(out), [None if p.grad is None else p.grad.detach().clone() for p in fn.model.parameters()]
    try:
        # frames / labels per batch; S <= 64 and hypothesis labels <= 16 throughout: one (S, U) bucket
        shapes = ((150, 6), (141, 5), (163, 7), (172, 6), (134, 4), (190, 8))
        worst_l2 = (0.0, -1, "")
        for k, (T_in_k, U_k) in enumerate(shapes):
            args = batch(5 + k % 3, 10 + k, T_in_k, U_k)
            got_loss, got = grads_of(step, args)
            want_loss, want = grads_of(ref_step, args)
            assert abs(got_loss - want_loss) <= 1e-4 * abs(want_loss) + 1e-5, (k, got_loss, want_loss)
            big = max(float(b.norm() / b.numel() ** 0.5) for b in want if b is not None)
            for (name, _), a, b in zip(net.named_parameters(), got, want):
                if b is None:
                    assert a is None or float(a.abs().max()) == 0.0, name
                    continue
                scale = float(b.abs().max()) + 1e-12
                d = float((a - b).abs().max())
                if k < 2:           # the eager launch sequence on the batch as it is
                    assert d <= 2e-3 * scale + 1e-7, (k, name, d, scale)
                    continue
                # a padded time axis sums the BatchNorm statistics in another row order, which may move a pre-activation within
                # 1e-7 of zero to the other side of a ReLU (tests/test_train_step_gpu.py::test_padded_time_axis_*: the same
                # per-entry bound).  In the L2 norm the padded calls match to rounding: the 3.8e-2 once allowed for here was
                # the risk term's 1/T taken from the padded axis (42 frames for 28 / 35), not ReLU flips
                assert d <= 0.3 * scale + 1e-7, (k, name, d, scale)
                if float(b.norm() / b.numel() ** 0.5) > 1e-4 * big:
                    worst_l2 = max(worst_l2, (float((a - b).norm() / b.norm()), k, name))
                    assert worst_l2[0] < MBR_NEVER_RECUR_L2_BOUND, worst_l2
        print("padded replays vs the eager step: worst relative L2 difference %.1e (call %d, %s)" % worst_l2)
        assert step.broken is None, step.broken
        # call 1 warm-up, 2 eager (first shape of bucket (192, 8) after the warm-up), 3 captures the bucket at (192, 8), 4-6 ride it
        assert step.stats.get("bucket_captures") == 1 and step.stats["captures"] == 1, step.stats
        assert step.stats["replays"] == 4 and step.stats["eager"] == 2 and step.stats.get("padded") == 3, step.stats
        assert [(k_[0][1], k_[2][1]) for k_ in step.entries] == [(192, 8)]
    finally:
        G.PRECISION = old
        step.close()
        ref_step.close()


MBR_NEVER_RECUR_L2_BOUND = 1.2e-4     # measured on MI355X: 3.8e-5 (5.5e-2 while the risk term took T from the padded axis)


# ---- risk_surrogate against the reference's own trajectory loops, in float64 -----------------------------------------
def reference_risk_grads(x, pred, hyps, seq_grad, blk, sm_scale, fc1, fc_gate, fc2):
    """Lines :197-235 of train_transducer_mbr_bmuf_otfaug.py restated on a GIVEN encoder output x (B, T, H) and prediction
    network output pred (B*beam, U, H): the Python trajectory loops, the dense one-hot `mbr_grad` (blank column / T, T =
    x.size(1)), `out.backward(mbr_grad)` -- in the arithmetic of the inputs (float64).  Returns the surrogate value
    sum(out * mbr_grad), its absolute-term scale and the gradients w.r.t. x, pred and the fc1 / fc_gate / fc2 weights and
    biases."""
    bsz, T, H = x.shape
    beam = len(hyps[0])
    bb = bsz * beam
    U = pred.shape[1]
    x = x.detach().clone().requires_grad_(True)
    pred = pred.detach().clone().requires_grad_(True)
    xe = x.unsqueeze(1).expand(-1, beam, -1, -1).contiguous().view(bb, -1, H)
    b_idx, x_idx, y_idx = [], [], []
    mbr_grad = x.new_zeros(bb, T + U, fc2.weight.shape[0])
    for i in range(bsz):
        for j in range(beam):
            h = [int(e) for e in hyps[i][j]]
            t_idx, u_idx = [0], [0]
            for t in range(1, len(h)):
                t_idx.append(t_idx[t - 1] + int(h[t - 1] == blk))
                u_idx.append(u_idx[t - 1] + int(h[t - 1] != blk))
            t_idx.extend((T + U - len(t_idx)) * [0])
            u_idx.extend((T + U - len(u_idx)) * [0])
            x_idx.extend(t_idx)
            y_idx.extend(u_idx)
            b_idx.extend([i * beam + j] * (T + U))
            mbr_grad[i * beam + j, torch.arange(len(h)), h] = seq_grad[i][j]
    joint = torch.cat((xe[b_idx, x_idx, :], pred[b_idx, y_idx, :]), dim=-1).view(bb, T + U, -1)
    out = fc2(torch.tanh(fc1(joint)) * torch.sigmoid(fc_gate(joint)))
    out = F.log_softmax(sm_scale * out, dim=-1)
    mbr_grad[:, :, blk] = mbr_grad[:, :, blk] / float(T)
    wrt = [x, pred, fc1.weight, fc1.bias, fc_gate.weight, fc_gate.bias, fc2.weight, fc2.bias]
    grads = torch.autograd.grad(out, wrt, grad_outputs=mbr_grad)
    terms = (out * mbr_grad).detach()
    return float(terms.sum()), float(terms.abs().sum()), dict(zip(RISK_WRT, grads))


RISK_WRT = ("enc", "pred", "fc1.weight", "fc1.bias", "fc_gate.weight", "fc_gate.bias", "fc2.weight", "fc2.bias")

# edge cases of the trajectories / log-softmax (every case also holds a hypothesis without labels -- its y row is all
# padding -- and one with exactly T blanks, whose last step reads frame T - 1)
RISK_CASES = {
    "blk0": dict(V=120, blk=0, sm=1.0, beam=3),
    "blk_last_sm08": dict(V=120, blk=119, sm=0.8, beam=3),
    "equal_distances": dict(V=120, blk=0, sm=0.9, beam=3, same_row=1),       # seq_grad row exactly 0 (kernel's v == 0)
    "beam1": dict(V=120, blk=7, sm=1.0, beam=1),
    "dead_rows": dict(V=120, blk=0, sm=0.9, beam=2, buckets=True),           # S / U padded to their buckets
    "V5001_generic_softmax": dict(V=5001, blk=5000, sm=0.8, beam=2),
    "V4096_wave": dict(V=4096, blk=0, sm=0.9, beam=2),
    "V5000_benchmarked": dict(V=5000, blk=0, sm=0.8, beam=2),
    "padded_enc": dict(V=120, blk=0, sm=0.9, beam=3, pad=5),
    "padded_enc_blk_last_buckets": dict(V=120, blk=119, sm=0.8, beam=2, pad=9, buckets=True),
}


def _risk_case(V, blk, sm, beam, same_row=None, buckets=False, pad=0, B=3, T=11, H=32, seed=0):
    """Float64 inputs of one risk_surrogate call: encoder output, fc1 / fc_gate / fc2, valid N-best lists (no label
    after the T-th blank), seq_grad, and the host arrays of pika_amd.mbr.hyp_arrays."""
    from pika_amd import mbr
    g = torch.Generator().manual_seed(seed)

    def lab(n):
        v = torch.randint(0, V - 1, (n,), generator=g)
        return (v + (v >= blk).long()).tolist()             # any symbol but blank
    hyps, targets = [], []
    for b in range(B):
        row = []
        shared = lab(4)
        for j in range(beam):
            k = b * beam + j
            if k == 0:
                nb, labs = T - 2, []                                            # no labels
            elif k == 1:
                nb, labs = T, lab(4)                                            # exactly T blanks
            else:
                nb, labs = T - int(torch.randint(0, 3, (1,), generator=g)), lab(int(torch.randint(1, 7, (1,), generator=g)))
            if b == same_row:
                labs = list(shared)
            at = set(torch.randperm(nb + len(labs), generator=g)[:len(labs)].tolist())    # label positions, in order
            it = iter(labs)
            seq = [next(it) if i in at else blk for i in range(nb + len(labs))]
            if nb == T and seq[-1] != blk:                  # a label after the T-th blank: no valid hypothesis
                i = max(i for i, e in enumerate(seq) if e == blk)
                seq[i], seq[-1] = seq[-1], seq[i]
            row.append([torch.tensor(e) for e in seq])
        hyps.append(row)
        targets.append(shared if b == same_row else lab(5))
    seq_grad = torch.randn(B, beam, generator=g, dtype=torch.float64)
    if same_row is not None:
        scores = torch.randn(B, beam, generator=g).tolist()
        tl = torch.tensor([len(t) for t in targets])
        tg = torch.full((B, max(tl)), V, dtype=torch.long)
        for b, t in enumerate(targets):
            tg[b, :len(t)] = torch.tensor(t)
        _, dist, sg, _ = mbr.risk_terms(hyps, scores, tg, tl, blk, "cpu")
        assert float(dist[same_row].abs().max()) == 0.0 and float(sg[same_row].abs().max()) == 0.0
        seq_grad[same_row] = sg[same_row].double()
    nonblk = [[[int(e) for e in h if int(e) != blk] for h in row] for row in hyps]
    S = Umax = None
    if buckets:
        u_need = max(len(h) for row in nonblk for h in row)
        S = -(-max(len(h) for row in hyps for h in row) // 32) * 32
        Umax = -(-max(u_need, 1) // 8) * 8
    y_h, sym_h, slen_h = mbr.hyp_arrays(hyps, nonblk, V, blk, S=S, Umax=Umax)
    if buckets:
        assert sym_h.shape[1] % 32 == 0 and (slen_h < sym_h.shape[1]).all()          # dead rows exist
    torch.manual_seed(seed + 1)
    fc1, fc_gate, fc2 = (torch.nn.Linear(2 * H, H).double(), torch.nn.Linear(2 * H, H).double(),
                         torch.nn.Linear(H, V).double())
    enc = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    pred = torch.randn(B * beam, y_h.shape[1] + 1, H, generator=g, dtype=torch.float64)
    garbage = 1e4 * torch.randn(B, pad, H, generator=g, dtype=torch.float64)     # large, finite
    return SimpleNamespace(hyps=hyps, seq_grad=seq_grad, y=y_h, sym=sym_h, slen=slen_h, fc1=fc1, fc_gate=fc_gate, fc2=fc2,
                           enc=enc, pred=pred, garbage=garbage, blk=blk, sm=sm, T=T, u_ref=max(len(h) for r in nonblk for h in r) + 1)


def _risk_native(c, device, dtype):
    """risk_surrogate on the case's inputs (a padded encoder output when the case asks for one, its valid length as a
    device tensor); returns the value and the gradients of RISK_WRT (the encoder gradient over the padded axis)."""
    import copy
    from pika_amd import mbr
    mods = [copy.deepcopy(m).to(device=device, dtype=dtype) for m in (c.fc1, c.fc_gate, c.fc2)]
    enc = torch.cat((c.enc, c.garbage), 1).to(device=device, dtype=dtype).requires_grad_(True)
    pred = c.pred.to(device=device, dtype=dtype).requires_grad_(True)
    y, sym, slen = (torch.from_numpy(a).to(device) for a in (c.y, c.sym, c.slen))

    def predict(yy):
        assert torch.equal(yy[:, 1:], y) and int(yy[:, 0].abs().max()) == 0
        return pred
    model = SimpleNamespace(predict=predict, fc1=mods[0], fc_gate=mods[1], fc2=mods[2])
    t_enc = torch.tensor([c.T], dtype=torch.int32, device=device) if c.garbage.shape[1] else None
    s = mbr.risk_surrogate(model, enc, y, sym, slen, c.seq_grad.to(device=device, dtype=dtype), c.blk, c.sm, t_enc=t_enc)
    wrt = [enc, pred] + [p for m in mods for p in (m.weight, m.bias)]
    grads = torch.autograd.grad(s, wrt)
    return float(s.detach()), {k: g.detach().double().cpu() for k, g in zip(RISK_WRT, grads)}


def _risk_errors(c, device, dtype):
    """(value error, {name: max |native - oracle| / max |oracle|}) of one case; the oracle runs in float64 on the inputs as
    the native side sees them (rounded to `dtype`), on the UNPADDED encoder output.  Asserts the padded frames' gradient
    and the unused prediction-network rows' gradient are exactly zero."""
    import copy
    rnd = (lambda t: t.to(dtype).double())
    mods = [copy.deepcopy(m) for m in (c.fc1, c.fc_gate, c.fc2)]
    for m in mods:
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(rnd(p))
    want_v, abs_v, want = reference_risk_grads(rnd(c.enc), rnd(c.pred)[:, :c.u_ref], c.hyps, rnd(c.seq_grad), c.blk, c.sm,
                                               *mods)
    got_v, got = _risk_native(c, device, dtype)
    T = c.T
    assert float(got["enc"][:, T:].abs().max() if got["enc"].shape[1] > T else 0.0) == 0.0, "gradient on padded frames"
    assert float(got["pred"][:, c.u_ref:].abs().max() if got["pred"].shape[1] > c.u_ref else 0.0) == 0.0
    got["enc"], got["pred"] = got["enc"][:, :T], got["pred"][:, :c.u_ref]
    errs = {}
    for k in RISK_WRT:
        sc = float(want[k].abs().max())
        errs[k] = float((got[k] - want[k]).abs().max()) / sc if sc > 0 else float(got[k].abs().max())
    return abs(got_v - want_v) / max(abs_v, 1e-300), errs, want


@pytest.mark.parametrize("case", sorted(RISK_CASES))
def test_cpu_risk_surrogate_equals_the_reference_loops_in_float64(case):
    """risk_surrogate (device trajectories, split joint, 1/T of the blank rows, clamp) against the reference's own loops
    and dense mbr_grad, both in float64: the value and every gradient to 1e-10 of the tensor's largest entry -- on a
    padded encoder output too (garbage frames of 1e4, the valid length as a tensor), whose padded frames get an exactly
    zero gradient."""
    c = _risk_case(**RISK_CASES[case])
    ev, errs, want = _risk_errors(c, "cpu", torch.float64)
    assert float(want["enc"].abs().max()) > 0 or c.seq_grad.abs().max() == 0
    assert ev <= 1e-10 and max(errs.values()) <= 1e-10, (ev, errs)


def test_cpu_risk_surrogate_on_a_padded_enc_takes_T_from_the_valid_length():
    """The blank rows of a padded encoder output are scaled by 1 / (valid length), not 1 / (padded length): the gradient
    of fc2.bias[blk] (mostly the blank rows' term) moves by about padded / valid T if the padded axis is taken for T."""
    from pika_amd import mbr
    c = _risk_case(**RISK_CASES["padded_enc"])
    _, _, want = _risk_errors(c, "cpu", torch.float64)
    _, got = _risk_native(c, "cpu", torch.float64)
    assert abs(float(got["fc2.bias"][c.blk] / want["fc2.bias"][c.blk]) - 1.0) < 1e-10
    # the eager call (no valid length) on the same padded tensor is off by (T + pad) / T on that entry
    enc = torch.cat((c.enc, c.garbage), 1).requires_grad_(True)
    model = SimpleNamespace(predict=lambda yy: c.pred, fc1=c.fc1, fc_gate=c.fc_gate, fc2=c.fc2)
    s = mbr.risk_surrogate(model, enc, *(torch.from_numpy(a) for a in (c.y, c.sym, c.slen)), c.seq_grad, c.blk, c.sm)
    g = torch.autograd.grad(s, [c.fc2.bias])[0]
    ratio = float(want["fc2.bias"][c.blk] / g[c.blk])
    assert abs(ratio / ((c.T + c.garbage.shape[1]) / c.T) - 1.0) < 0.05, ratio      # (1.466 for 16 / 11 frames)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "mixed"])
@pytest.mark.parametrize("case", sorted(RISK_CASES))
def test_gpu_risk_surrogate_equals_the_reference_loops(hip_device, mode, case):
    """The same cases on the device (MFMA GEMMs, pika_log_softmax_rows' wave / generic kernels, the risk-gradient
    kernel) against the float64 oracle: fp32 to 1e-4 of each tensor's largest entry; "mixed" (two-term products forward,
    bf16 backward products) to RISK_MIXED_BOUND, measured on MI355X (the printed line)."""
    from pika_amd import gemm as G
    c = _risk_case(**RISK_CASES[case])
    old, G.PRECISION = G.PRECISION, mode
    try:
        ev, errs, _ = _risk_errors(c, hip_device, torch.float32)
    finally:
        G.PRECISION = old
    worst = max(errs, key=errs.get)
    print("risk_surrogate %s %s: value %.1e, worst gradient %.1e of its scale (%s)" % (case, mode, ev, errs[worst], worst))
    bound = 1e-4 if mode == "fp32" else RISK_MIXED_BOUND
    assert ev <= bound and errs[worst] <= bound, (ev, errs)


RISK_MIXED_BOUND = 2e-2     # measured on MI355X: <= 7.8e-3 (beam1, fc_gate.weight), value <= 8.1e-8


def _scale_of(grads, n):
    """A gradient's scale: its largest entry -- or, for a bias, its weight's if that is larger (a bias whose gradient is
    mathematically zero holds rounding noise only, see _worst)."""
    own = float(grads[n].abs().max())
    sib = n[:-4] + "weight" if n.endswith(".bias") else None
    return max(own, float(grads[sib].abs().max()) if sib in grads else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("rnnt_scale", [0.1, 0.0])
@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_gpu_graphed_mbr_padded_replays_give_the_gradients_of_the_unpadded_batch(hip_device, mode, rnnt_scale):
    """Three calls of ONE bucket graph of GraphedMbrStep (captured at 192 frames x 8 labels): the capture call itself
    (163 frames: padded), a replay on 134 frames (padded, another encoder length) and a replay on 192 frames (the bucket's
    own length) -- each against `eager_step` on the unpadded batch, parameter by parameter.  rnnt_scale 0 leaves the risk
    term alone.  blk = V - 1; every N-best holds a hypothesis without labels and one with exactly T blanks (T = the batch's
    own encoder length).  Parameters after the encoder depend on it through its forward values only: to
    MBR_PADDED_POST_BOUND of their scale; encoder parameters to the bounds of the other padded tests (a ReLU flip switches
    single entries).  While the risk term took T from the padded axis, fc2.bias[blk] and the blank column of fc2 were off by
    about padded / own T (42 / 35, 42 / 28) on the padded calls, the capture call included."""
    import copy
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pika_amd", "dropin"))
    from oracle.pika_ref import seeded_state_dict
    from model.transducer import Net
    from pika_amd import gemm as G
    from pika_amd import mbr
    V, B, beam = 120, 3, 3
    blk = V - 1
    opt = SimpleNamespace(rnn_size=64, local_rank=0, decoder_type="transformer", brnn=False, encoder_type="tdnn",
                          dropout=0.0, enc_layers=2, dec_layers=1, embd_dim=32, padding_idx=V)
    net = Net(opt, 240, V)
    net.encoder = type(net.encoder)(240, 0, 64, tdnn_nhid=64, tdnn_layers=6)
    net.pack_seq = False
    sd = seeded_state_dict(net, 78)
    sd["fc2.bias"][blk] -= 4.0          # a rare blank: fc2.bias[blk] is then mostly the blank rows' term, which carries 1/T
    net.load_state_dict(sd)
    net = net.to(hip_device).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0

    def batch(seed, T_in, U):
        Tp = (T_in - 24 + 3) // 4                               # the batch's own encoder length
        gg = torch.Generator().manual_seed(seed)
        feats = torch.randn(B, T_in, 240, generator=gg).to(hip_device)
        labels = torch.randint(0, V - 1, (B, U), generator=gg)  # (no blank: blk = V - 1)
        ali = torch.tensor([U, U - 1, max(U - 2, 1)], dtype=torch.int32)
        for b in range(B):
            labels[b, int(ali[b]):] = V
        hyps, scores = [], []
        for b in range(B):
            row, sc = [], []
            for j in range(beam):
                nl = 0 if j == 0 else int(torch.randint(1, 9, (1,), generator=gg))
                nb = Tp if j == 1 else Tp - int(torch.randint(0, 3, (1,), generator=gg))
                labs = torch.randint(0, V - 1, (nl,), generator=gg).tolist()
                at = set(torch.randperm(nb + nl - 1, generator=gg)[:nl].tolist())   # labels in order, the last symbol a
                it = iter(labs)                                                      # blank: no label after the T-th
                sym = [next(it) if i in at else blk for i in range(nb + nl - 1)] + [blk]
                row.append([torch.tensor(e) for e in sym])
                sc.append(torch.tensor(-1.0 - 0.3 * j - 0.01 * float(torch.rand(1, generator=gg))))
            hyps.append(row)
            scores.append(sc)
        x_len = torch.full((B,), Tp, dtype=torch.int32)
        return feats, labels.to(hip_device), x_len.to(hip_device), ali.to(hip_device), hyps, scores

    old, G.PRECISION = G.PRECISION, mode
    step = mbr.GraphedMbrStep(net, rnnt_scale=rnnt_scale, sm_scale=0.9, blk=blk, min_seen=2, warmup=1, s_bucket=64,
                              u_bucket=16)
    ref_step = mbr.GraphedMbrStep(copy.deepcopy(net), rnnt_scale=rnnt_scale, sm_scale=0.9, blk=blk)

    def grads_of(fn, args):
        fn.model.zero_grad(set_to_none=True)
        out = fn(*args) if fn is step else fn.eager_step(*args)
        torch.cuda.synchronize()
        return float(out), {n: p.grad.detach().clone() for n, p in fn.model.named_parameters() if p.grad is not None}
    try:
        # warm-up (eager), the bucket's first shape (eager), its second: captured at (192, 8) and replayed padded, then a
        # padded replay with another encoder length, then a replay at the bucket's own length
        shapes = ((150, 6), (141, 5), (163, 7), (134, 4), (192, 8))
        for k, (T_in, U) in enumerate(shapes):
            args = batch(20 + k, T_in, U)
            got_loss, got = grads_of(step, args)
            want_loss, want = grads_of(ref_step, args)
            assert set(got) == set(want)
            assert abs(got_loss - want_loss) <= 1e-4 * abs(want_loss) + 1e-5, (k, got_loss, want_loss)
            # the blank entries first: fc2.bias[blk] and the blank column of fc2 (its weight row) carry the 1/T of the blank rows;
            # measured against themselves (sums with cancellation: fp32 rounding reaches 7e-5 of fc2.bias[blk]) to 1e-3 at
            # least -- the padded axis taken for T moves them by 10-20 %
            for n in ("fc2.bias", "fc2.weight"):
                a, b = got[n][blk], want[n][blk]
                e = float((a - b).abs().max() / b.abs().max())
                assert e <= max(MBR_PADDED_POST_BOUND[mode], 1e-3), (k, n + "[blk]", e, "ratio %.3f" % float(a.norm() / b.norm()))
            rms = {n: float(w.norm() / w.numel() ** 0.5) for n, w in want.items()}
            post, enc, l2 = (0.0, ""), (0.0, ""), (0.0, "")
            for n in want:
                e = float((got[n] - want[n]).abs().max()) / (_scale_of(want, n) + 1e-12)
                if n.startswith("encoder."):
                    enc = max(enc, (e, n))
                    if rms[n] > 1e-4 * max(rms.values()):
                        l2 = max(l2, (float((got[n] - want[n]).norm() / want[n].norm()), n))
                else:
                    post = max(post, (e, n))
            print("graphed MBR %s rnnt_scale %.1f, call %d (%d frames, %s): after the encoder %.1e of scale (%s); encoder %.1e "
                  "(%s), relative L2 %.1e (%s)" % (mode, rnnt_scale, k + 1, T_in, "replay" if k >= 2 else "eager",
                                                   post[0], post[1], enc[0], enc[1], l2[0], l2[1]))
            assert post[0] <= MBR_PADDED_POST_BOUND[mode], (k, post)
            assert enc[0] <= 0.3 and l2[0] < MBR_PADDED_L2_BOUND[mode], (k, enc, l2)
        assert step.broken is None, step.broken
        assert step.stats.get("bucket_captures") == 1 and step.stats["captures"] == 1, step.stats
        assert step.stats["replays"] == 3 and step.stats["eager"] == 2 and step.stats.get("padded") == 1, step.stats
        assert [(k_[0][1], k_[2][1]) for k_ in step.entries] == [(192, 8)]
    finally:
        G.PRECISION = old
        step.close()
        ref_step.close()


# measured on MI355X, worst over the five calls and both rnnt_scale values -- parameters after the encoder, per entry: fp32
# 4.9e-6, mixed 2.5e-3 (one bf16 rounding step, 2^-9, of a backward product lands differently in the two runs);
# encoder parameters, relative L2: fp32 6.6e-6 (held to the never-recur test's bound), mixed 1.1e-2 (test_padded_time_axis_*)
MBR_PADDED_POST_BOUND = {"fp32": 5e-5, "mixed": 5e-3}
MBR_PADDED_L2_BOUND = {"fp32": MBR_NEVER_RECUR_L2_BOUND, "mixed": 5e-2}


def test_cpu_encoder_valid_out_is_the_output_length_of_the_unpadded_batch():
    """encoder.valid_out (what GraphedMbrStep derives the risk term's T from on a padded time axis) equals the time axis
    the encoder returns for a batch of that many frames -- the reference's T = x.size(1) (:140)."""
    from pika_amd.model.encoder import Net as Encoder
    for layers in (5, 6, 9):
        enc = Encoder(40, 0, 16, tdnn_nhid=16, tdnn_layers=layers).eval()
        for T in (61, 62, 63, 64, 97, 134, 163):
            with torch.no_grad():
                want = enc(torch.randn(2, T, 40)).shape[1]
            assert int(enc.valid_out(torch.tensor([T], dtype=torch.int32))) == want, (layers, T, want)
