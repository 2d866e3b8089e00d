"""Audio classification end to end on the GPU (huggingface/classification.py, csrc/seq_cls.hip): random tiny `...ForSequenceClassification`
models of transformers behind classifier_from_huggingface against transformers' own f32 logits on the CPU, with config.use_weighted_layer_sum
off and -- where the plan exposes its hidden states -- on.

Bound: pool, layer sum and projector are linear, so with M = cls_w proj_w a deviation of at most eps in every element of the (weighted) hidden
state moves logit l by at most eps sum_j |M[l][j]| (a mean of elements each within eps is within eps).  eps is what the encoder tests grant
that plan's last_hidden_state: atol 5e-4 + rtol 1e-4 under precision="fp32" (taken at the reference's largest hidden-state magnitude),
max 0.1 under "bf16"."""
import copy

import pytest
import torch

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu

# the tiny configurations of tests/test_gpu_family_finetune.py, test_gpu_wavlm.py, test_gpu_sew.py and test_gpu_conformer.py (copied: those files
# are not imported)
BASE = dict(vocab_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, conv_dim=(32, 32, 32),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, hidden_dropout=0.0,
            activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
            mask_feature_prob=0.0)
WIDE = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32,) * 7,
            conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
            pad_token_id=0)
SEW = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=32, conv_dim=(32, 32, 32, 32, 64),
           conv_kernel=(10, 3, 1, 3, 1), conv_stride=(5, 2, 1, 2, 1), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, squeeze_factor=2,
           layer_norm_eps=1e-3, pad_token_id=0, feat_extract_norm="group")
# name: (transformers class prefix, config, samples per clip, trained with an attention mask, the plan taps its hidden states)
CASES = {
    "wav2vec2_group_postln": ("Wav2Vec2", dict(BASE, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False), 4000, False, True),
    "wav2vec2_layer_preln_masked": ("Wav2Vec2", dict(BASE, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True), 4000, True, True),
    "hubert": ("Hubert", dict(BASE, feat_proj_layer_norm=False, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False), 4000, False, True),
    "wavlm": ("WavLM", dict(WIDE, feat_extract_norm="group", do_stable_layer_norm=False, num_buckets=32, max_bucket_distance=40), 75 * 320 + 80, False, True),
    "data2vec_audio": ("Data2VecAudio", dict(BASE, num_conv_pos_embeddings=3, conv_pos_kernel_size=19), 4000, False, True),
    "unispeech_sat": ("UniSpeechSat", dict(BASE, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True), 4000, False, True),
    "sew": ("SEW", SEW, 4000, False, False),
    "conformer_rotary": ("Wav2Vec2Conformer", dict(WIDE, position_embeddings_type="rotary", conv_depthwise_kernel_size=31, layer_norm_eps=1e-3,
                                                   feat_extract_norm="group"), 75 * 320 + 80, False, False),
}
LABELS = ["yes", "no", "up", "down", "left", "right", "on"]
PROJ = 48
RAGGED = [4000, 3000, 2111]
PARAMS = [(name, weighted) for name, case in CASES.items() for weighted in (False, True) if case[4] or not weighted]


def _random_model(name, weighted, seed=5):
    cls, cfg, _, _, _ = CASES[name]
    torch.manual_seed(seed)
    config = getattr(transformers, cls + "Config")(**cfg, classifier_proj_size=PROJ, num_labels=len(LABELS), use_weighted_layer_sum=weighted,
                                                    id2label=dict(enumerate(LABELS)), label2id={s: i for i, s in enumerate(LABELS)})
    model = getattr(transformers, cls + "ForSequenceClassification")(config).eval()
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_mean"):                              # the conformer's BatchNorm: random statistics and affine
                v.copy_(0.3 * torch.randn_like(v))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand_like(v))
            elif k.endswith("batch_norm.weight"):
                v.copy_(1.0 + 0.2 * torch.randn_like(v))
            elif cls == "SEW" and "pos_conv_embed" in k and not k.endswith(".bias"):
                v.copy_(0.5 + torch.rand_like(v) if v.shape[0] == 1 and v.shape[1] == 1 else 0.3 * torch.randn_like(v))
            elif k.endswith("upsample.projection.weight"):
                v.copy_(torch.randn_like(v) * v.shape[1] ** -0.5)
            elif k.endswith("rel_attn_embed.weight"):
                v.copy_(1.5 * torch.randn_like(v))
            elif k.endswith("gru_rel_pos_const"):
                v.copy_(1.0 + 0.5 * torch.randn_like(v))
            elif k.endswith("gru_rel_pos_linear.weight"):
                v.copy_(0.1 * torch.randn_like(v))
            elif k.endswith(".bias"):
                v.copy_(0.1 * torch.randn_like(v))
        for head in (model.projector, model.classifier):               # logits of order 1 to 10 instead of transformers' 0.02-scale start
            head.weight.copy_(2.0 * torch.randn_like(head.weight) / head.weight.shape[1] ** 0.5)
        if weighted:
            model.layer_weights.copy_(torch.randn_like(model.layer_weights))
    return model


_WORLDS = {}


def _world(name, weighted):
    """The model, its input and transformers' f32 logits on the CPU: computed once per case, shared by both precisions, never changed."""
    key = (name, weighted)
    if key in _WORLDS:
        return _WORLDS[key]
    _, _, n, masked, _ = CASES[name]
    model = _random_model(name, weighted)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, n, generator=g)
    lengths = torch.tensor(RAGGED if masked else [n] * 3)
    xn = torch.zeros_like(x)
    for i, li in enumerate(lengths.tolist()):                           # Wav2Vec2FeatureExtractor: zero mean, unit variance over the valid samples
        xn[i, :li] = (x[i, :li] - x[i, :li].mean()) / torch.sqrt(x[i, :li].var(unbiased=False) + 1e-7)
        x[i, li:] = 0
    am = (torch.arange(n)[None, :] < lengths[:, None]).long() if masked else None
    with torch.no_grad():
        out = model(xn, attention_mask=am, output_hidden_states=True)
        m_abs = (model.classifier.weight.double() @ model.projector.weight.double()).abs().sum(1)      # sum_j |M[l][j]|
    hs = out.hidden_states if weighted else (out.hidden_states[-1],)
    w = dict(model=model, x=x, lengths=lengths, ref=out.logits.double(), m_abs=m_abs, h_max=max(float(h.abs().max()) for h in hs))
    assert len(out.hidden_states) == model.config.num_hidden_layers + 1
    _WORLDS[key] = w
    return w


def _module(w, masked, precision):
    from thunder_speech_amd.huggingface import classifier_from_huggingface
    m = classifier_from_huggingface(copy.deepcopy(w["model"]), transformers.Wav2Vec2FeatureExtractor(return_attention_mask=masked))
    m.encoder.precision = precision
    return m.cuda()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,weighted", PARAMS)
def test_logits_match_transformers_and_the_graph_equals_the_eager_run(name, weighted, precision):
    masked = CASES[name][3]
    w = _world(name, weighted)
    m = _module(w, masked, precision)
    x, lengths = w["x"].cuda(), w["lengths"].cuda()
    with torch.no_grad():
        logits = m(x, lengths)
    assert logits.shape == (3, len(LABELS)) and logits.dtype == torch.float32
    eps = 5e-4 + 1e-4 * w["h_max"] if precision == "fp32" else 0.1
    err = (logits.double().cpu() - w["ref"]).abs()
    bound = eps * w["m_abs"][None, :]
    print(f"{name} weighted={weighted} {precision}: max |dlogit| {float(err.max()):.3e}, max err/bound {float((err / bound).max()):.4f}, "
          f"logit scale {float(w['ref'].abs().max()):.2f}, max |h| {w['h_max']:.2f}")
    assert bool((err <= bound).all())
    if masked:                                                          # the ragged clips pooled over their own frames: not over all of them
        with torch.no_grad():
            full = m(x, torch.full_like(lengths, x.shape[1]))
        assert float((full[1:] - logits[1:]).abs().max()) > 2 * float(err.max())

    # labels: wherever the reference's margin exceeds twice the deviation measured above (under fp32 that must be every clip)
    dev = float(err.max())
    top = w["ref"].topk(len(LABELS), dim=1)
    clear = (top.values[:, 0] - top.values[:, 1]) > 2 * dev
    assert bool(clear.all()) if precision == "fp32" else True
    full_len = not masked                                               # predict() treats every clip as full length
    if full_len:
        lengths = lengths.to(torch.int32)                               # predict()'s own lengths tensor: one signature, one graph
        eager = m._forward_eager(x, lengths)
        m.graph_inference = True
        labels = m.predict(x)
        graphs = m.__dict__["_graphs"]
        assert graphs[1].count() == 1
        for a, b in zip(m._graphed(x, lengths), eager):
            assert torch.equal(a, b)                                    # the replayed graph: equal bits
        assert m.__dict__["_graphs"] is graphs and graphs[1].count() == 1
        m.graph_inference = False
        assert m.predict(x) == labels
        for i in range(3):
            if bool(clear[i]):
                assert labels[i] == LABELS[int(top.indices[i, 0])]
        assert eager[1].tolist() == eager[0].argmax(1).tolist()
        assert torch.allclose(eager[2], torch.log_softmax(eager[0], 1).max(1).values, atol=1e-5)
        topk = m.predict_topk(x, 3)
        want_p = torch.softmax(w["ref"], 1)
        for i in range(3):
            assert [s for s, _ in topk[i]] == [LABELS[j] for j in eager[0][i].topk(3).indices.tolist()]
            for s, q in topk[i]:
                assert abs(q - float(want_p[i, LABELS.index(s)])) <= 2 * dev + 1e-6
        if weighted:
            # a changed layer weight reaches the captured graph through the soft-max buffer: no re-capture, and the eager run's bits
            m.graph_inference = True
            with torch.no_grad():
                m.layer_weights.copy_(torch.tensor([1.5, -0.5, 0.25], device="cuda")[: m.layer_weights.shape[0]])
            after = [t.clone() for t in m._graphed(x, lengths)]
            assert m.__dict__["_graphs"] is graphs and graphs[1].count() == 1
            assert not torch.equal(after[0], eager[0])
            for a, b in zip(after, m._forward_eager(x, lengths)):
                assert torch.equal(a, b)
    else:
        with torch.no_grad():
            assert m.predict(x) == [LABELS[i] for i in m(x, torch.full_like(lengths, x.shape[1])).argmax(1).tolist()]
