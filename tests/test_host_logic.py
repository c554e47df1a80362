"""CPU-side tests: the C-ABI library loads and exports every symbol include/capdec.h declares,
the host façade mirrors the reference surface, shard/gather index math (gloo, world_size 2),
and the product path fails loudly without a GPU (no CPU fallback)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from capdec_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_exports_every_header_symbol():
    from capdec_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build()
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    # what only the measurement build declares (#ifdef CAPDEC_MEASURE ... #endif) must NOT be in the shipped library
    measure_only = set(re.findall(r"\b(capdec_[a-z0-9_]+)\s*\(", " ".join(re.findall(r"#ifdef CAPDEC_MEASURE(.*?)#endif", header, flags=re.S))))
    assert measure_only == set(_capi.MEASURE_SIGNATURES) == {"capdec_set_debug_diverge"}
    header = re.sub(r"#ifdef CAPDEC_MEASURE.*?#endif", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(capdec_[a-z0-9_]+)\s*\(", header))
    declared -= {"capdec_ctx"}
    assert len(declared) >= 25
    assert declared == set(_capi.SIGNATURES), declared ^ set(_capi.SIGNATURES)
    lib = _capi.load_library()                      # binds every symbol or raises
    for name in declared:
        assert hasattr(lib, name)
    assert lib.capdec_abi_version() == _capi.ABI_VERSION == int(re.search(r"#define CAPDEC_ABI_VERSION (\d+)", header).group(1))
    # the library is built for gfx950 and links the HIP runtime only (no torch types in the ABI)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and "capdec_" in l.split()[-1][:7]}
    assert declared == exported, declared ^ exported           # nothing undeclared leaves the library: no debug hooks
    # ... and no measurement code is compiled in: no ablation / override knob is even named in the binary
    strs = subprocess.run(["strings", _capi.LIB_PATH], capture_output=True, text=True).stdout
    knobs = set(re.findall(r"CAPDEC_[A-Z0-9_]+", strs))
    # (the ablations and overrides of rounds 2-6 are retired: a knob the binary names is one that config.h documents)
    documented = set(re.findall(r"CAPDEC_[A-Z0-9_]+", open(os.path.join(ROOT, "capdec_amd", "csrc", "config.h")).read()))
    assert not {k for k in knobs if "ABL" in k or "STAMPS" in k}, knobs
    assert {k for k in knobs if not k.startswith("CAPDEC_ACT_")} <= documented, knobs - documented
    # the measurement library is the product library plus the diverged-beam hook and nothing else: one more exported
    # symbol, the very same environment knobs
    mlib = build.build(measure=True, verbose=False)
    assert mlib == _capi.MEASURE_LIB_PATH
    mout = subprocess.run(["nm", "-D", "--defined-only", mlib], capture_output=True, text=True).stdout
    mexported = {l.split()[-1] for l in mout.splitlines() if " T " in l and "capdec_" in l.split()[-1][:7]}
    assert mexported == exported | {"capdec_set_debug_diverge"}, mexported ^ exported
    mstrs = subprocess.run(["strings", mlib], capture_output=True, text=True).stdout
    assert set(re.findall(r"CAPDEC_[A-Z0-9_]+", mstrs)) == knobs


def test_ctypes_signatures_match_header_prototypes():
    """every prototype of include/capdec.h and its ctypes binding agree on the number of parameters and on which of
    them are pointers / integers / floats (an ABI drift between header, library and Python host would otherwise only
    show up as garbage on the GPU box)"""
    import ctypes as C
    from capdec_amd import _capi
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)                       # strip comments
    header = re.sub(r"#ifdef CAPDEC_MEASURE.*?#endif", " ", header, flags=re.S)   # (measurement builds only)
    protos = re.findall(r"\b(?:int|void|const char \*)\s*(capdec_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
    seen = 0
    for name, params in protos:
        params = " ".join(params.split())
        plist = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
        res, argtypes = _capi.SIGNATURES[name]
        assert len(plist) == len(argtypes), (name, plist, argtypes)
        for ptxt, at in zip(plist, argtypes):
            is_ptr = "*" in ptxt
            at_ptr = at in (C.c_void_p, C.c_char_p) or hasattr(at, "contents") or issubclass(at, C._Pointer)
            assert is_ptr == at_ptr, (name, ptxt, at)
            if not is_ptr:
                if re.search(r"\bfloat\b", ptxt):
                    assert at is C.c_float, (name, ptxt, at)
                elif re.search(r"\bsize_t\b|\buint64_t\b", ptxt):
                    assert at in (C.c_size_t, C.c_uint64), (name, ptxt, at)
                else:
                    assert at in (C.c_int, C.c_int32), (name, ptxt, at)
        seen += 1
    assert seen == len(_capi.SIGNATURES), (seen, len(_capi.SIGNATURES))


def test_ctypes_structs_match_header_layout(tmp_path):
    """every weight struct of include/capdec.h and its ctypes mirror agree on size, field names, field order and field
    offsets as the C compiler lays them out (gcc on a generated program that prints sizeof / offsetof)"""
    import ctypes as C
    from capdec_amd import _capi
    pairs = {"capdec_gpt2_layer": _capi.Gpt2Layer, "capdec_gpt2_weights": _capi.Gpt2Weights,
             "capdec_tmapper_layer": _capi.TMapperLayer, "capdec_tmapper_weights": _capi.TMapperWeights,
             "capdec_clip_block": _capi.ClipBlock, "capdec_clip_text_weights": _capi.ClipTextWeights,
             "capdec_clip_vision_weights": _capi.ClipVisionWeights, "capdec_conv_bn": _capi.ConvBn,
             "capdec_clip_resnet_weights": _capi.ClipResNetWeights}
    header = open(os.path.join(ROOT, "include", "capdec.h")).read()
    declared = set(re.findall(r"^}\s*(capdec_[a-z0-9_]+);", header, flags=re.M))
    assert declared == set(pairs), declared ^ set(pairs)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "capdec.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)   # unknown field -> compile error
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, val = line.split()
        cls = pairs[cname]
        if what == "size":
            assert C.sizeof(cls) == int(val), (cname, C.sizeof(cls), val)
        else:
            assert getattr(cls, what).offset == int(val), (cname, what, getattr(cls, what).offset, val)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values())
    # the header has no field the mirror lacks: count the declarators of each struct body
    for cname, cls in pairs.items():
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\}\s*" + cname + ";", re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.S).group(1)
        n_decl = sum(len(stmt.split(",")) for stmt in body.split(";") if stmt.strip())
        assert n_decl == len(cls._fields_), (cname, n_decl, len(cls._fields_))


def test_every_device_buffer_of_the_context_is_released_by_destroy():
    """capdec_destroy frees the context's grow-only device buffers from an explicit list: a buffer added to capdec_ctx
    (context.h) and forgotten there leaks once per context"""
    import re
    csrc = os.path.join(ROOT, "capdec_amd", "csrc")
    ctx = open(os.path.join(csrc, "context.h")).read()
    body = ctx[ctx.index("struct capdec_ctx {"):]
    names = []
    for decl in re.findall(r"^\s*DBuf\s+([^;]+);", body, flags=re.M):
        names += [n.strip() for n in decl.split(",")]
    assert len(names) > 60 and "lmflag" in names and "kc" in names
    destroy = open(os.path.join(csrc, "capi_context.hip")).read()
    destroy = destroy[destroy.index("void capdec_destroy("):]
    destroy = destroy[:destroy.index("\n}\n")]
    missing = [n for n in names if f"&c->{n}" not in destroy and f"c->{n}.release()" not in destroy]
    assert not missing, missing


def test_three_candidates_per_tile_flag_criterion_is_exact():
    """The rule behind the fused lm_head's second pass (select.hip: topk_merge_k3_kernel), restated in numpy and checked
    against brute force: keep the 3 best (value desc, column asc) of every 128-column tile, take the top 5 of what was
    kept, flag the row iff some tile's THIRD kept candidate is strictly better than that fifth.  Claim: an unflagged
    row's top 5 of the kept candidates IS its true top 5 -- also with many exactly equal logits (the tie rule is part of
    the order) and with a ragged last tile"""
    rng = np.random.default_rng(0)
    V, TILE, KEEP, K = 1531, 128, 3, 5
    nt = (V + TILE - 1) // TILE
    flagged = exact_unflagged = 0
    for trial in range(400):
        if trial % 2:      # few distinct values: ties everywhere
            x = rng.integers(0, 6, V).astype(np.float32)
        else:              # a cluster of large values inside one tile now and then
            x = rng.standard_normal(V).astype(np.float32)
            if trial % 4 == 0:
                t0 = int(rng.integers(0, nt)) * TILE
                x[t0 + rng.integers(0, min(TILE, V - t0), 4)] += 3.0
        order = np.lexsort((np.arange(V), -x))                 # value descending, column ascending
        truth = order[:K]
        rank = np.empty(V, np.int64); rank[order] = np.arange(V)     # position in the total order: smaller = better
        kept, thirds = [], []
        for t in range(nt):
            cols = np.arange(t * TILE, min(V, (t + 1) * TILE))
            best = cols[np.argsort(rank[cols])][:KEEP]
            kept += best.tolist()
            if len(best) == KEEP:
                thirds.append(best[-1])
        kept = np.array(kept)
        top = kept[np.argsort(rank[kept])][:K]
        flag = any(rank[c] < rank[top[-1]] for c in thirds)
        if flag:
            flagged += 1
        else:
            exact_unflagged += 1
            np.testing.assert_array_equal(top, truth)
        if not np.array_equal(top, truth):
            assert flag                                        # every row the 3-per-tile lists get wrong is flagged
    assert flagged > 20 and exact_unflagged > 100, (flagged, exact_unflagged)


def test_train_facade_schedule_and_tensor_names(golden):
    """host side of the train step (capdec_amd/train.py): the scheduler object walks the lr sequence the real transformers
    scheduler produced for the fixture (set at construction like LambdaLR, advanced by step()), AdamW carries the
    transformers-4.24 defaults, and the device's tensor order names exactly the reference model's parameters"""
    from capdec_amd import train as Tr
    from capdec_amd.engine import Engine
    g = golden("train_step_tm_tiny")
    opt = Tr.AdamW(None, lr=float(g["lr"]))
    assert opt.param_groups[0]["eps"] == 1e-6 and opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[0]["betas"] == (0.9, 0.999)
    sched = Tr.get_linear_schedule_with_warmup(opt, int(g["warmup"]), int(g["total"]))
    for want in g["lrs"]:
        assert abs(opt.param_groups[0]["lr"] - float(want)) < 1e-12
        opt.step()
        sched.step()
    assert sched.get_last_lr() == [opt.param_groups[0]["lr"]]
    ref_names = sorted(str(n)[len("clip_project."):] for n in g["names"])
    assert sorted(Engine.train_tensor_names("transformer", 3)) == ref_names and len(ref_names) == 3 + 12 * 3
    assert sorted("clip_project." + n for n in Engine.train_tensor_names("mlp")) == sorted(str(n) for n in golden("train_step_tiny")["names"])
    with pytest.raises(Exception):
        Tr.AdamW(None, lr=1e-3, correct_bias=False)


@pytest.mark.parametrize("mapping", ["mlp", "transformer_encoder"])
def test_trained_tensors_are_pulled_back_into_the_state_dict(mapping):
    """after train steps the mapper lives on the device: ``state_dict()`` (what the reference saves, train.py:359-371)
    must read every trained tensor back under its checkpoint name, in the device's slot order, exactly once -- checked
    with a stand-in for the engine that returns tensor number i filled with i"""
    from capdec_amd.gpt2_prefix import ClipCaptionPrefix, MappingType
    dims, nlay = synth.GPT2_TINY, 2
    mt = MappingType.MLP if mapping == "mlp" else MappingType.TransformerEncoder
    model = ClipCaptionPrefix(10, clip_length=10, prefix_size=512, num_layers=nlay, mapping_type=mt, gpt2_dims=dims)
    sd = synth.hot_state_dict(42, mapping, 512, 10, 10, nlay, dims)
    model.load_state_dict(sd)

    class FakeEngine:
        def __init__(self):
            self.calls = 0

        def mapper_parameters(self, shapes):
            self.calls += 1
            return {k: torch.full(shp, float(i)) for i, (k, shp) in enumerate(shapes.items())}

    fake = FakeEngine()
    model._engine, model._dirty = fake, False
    assert list(model.state_dict()) == list(sd) or set(model.state_dict()) == set(sd)
    assert fake.calls == 0                                   # nothing trained yet: the host copy is current
    model._device_ahead = True
    out = model.state_dict()
    assert fake.calls == 1 and not model._device_ahead
    names = list(model._train_shapes())
    assert all(n.startswith("clip_project.") for n in names) and len(names) == (4 if mapping == "mlp" else 3 + 12 * nlay)
    assert sorted(names) == sorted(k for k in sd if k.startswith("clip_project."))
    for i, n in enumerate(names):
        assert out[n].shape == sd[n].shape and bool((out[n] == float(i)).all()), n
        assert model.clip_project._sd[n[len("clip_project."):]] is out[n]
    for k in sd:
        if not k.startswith("clip_project."):
            assert torch.equal(out[k], sd[k])                # GPT-2 untouched in the frozen scope
    model.state_dict()
    assert fake.calls == 1
    model._engine = None


def test_no_cpu_fallback_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from capdec_amd._capi import CapdecError
    from capdec_amd.engine import Engine
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    from capdec_amd import synth
    with pytest.raises(CapdecError):
        Engine(0)
    m = ClipCaptionModel(10, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=synth.GPT2_TINY)
    m.load_state_dict(synth.hot_state_dict(1, "mlp", 512, 10, dims=synth.GPT2_TINY))
    with pytest.raises(CapdecError):
        m.clip_project(torch.zeros(1, 512))        # needs the HIP device: must raise, never compute on CPU


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "capdec_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("no oracle", ""), f"{f} mentions the oracle"


def test_facade_surface_matches_reference_names():
    from capdec_amd import gpt2_prefix, gpt2_prefix_eval, predictions_runner, train, transformer_mapper, synth
    MT = gpt2_prefix.MappingType
    assert MT('mlp') is MT.MLP and MT('transformer_encoder') is MT.TransformerEncoder
    assert MT.Transformer is MT.TransformerEncoder and train.MappingType is MT
    for name in ("generate_beam", "generate2"):
        assert getattr(predictions_runner, name) is getattr(gpt2_prefix_eval, name)
    import inspect
    sig = inspect.signature(gpt2_prefix_eval.generate_beam)
    assert list(sig.parameters) == ["model", "tokenizer", "beam_size", "prompt", "embed", "entry_length", "temperature", "stop_token"]
    assert sig.parameters["beam_size"].default == 5 and sig.parameters["entry_length"].default == 67
    sig = inspect.signature(gpt2_prefix_eval.generate2)
    assert list(sig.parameters) == ["model", "tokenizer", "tokens", "prompt", "embed", "entry_count", "entry_length",
                                    "top_p", "temperature", "stop_token"]
    sig = inspect.signature(train.noise_injection)
    assert list(sig.parameters)[:5] == ["x", "variance", "modality_offset", "uniform_noise", "dont_norm"]
    assert sig.parameters["variance"].default == 0.001
    sig = inspect.signature(gpt2_prefix.ClipCaptionModel.__init__)
    assert list(sig.parameters)[1:6] == ["prefix_length", "clip_length", "prefix_dim", "num_layers", "mapping_type"]
    assert sig.parameters["prefix_dim"].default == 640
    m = gpt2_prefix.ClipCaptionModel(10, prefix_dim=512, mapping_type=MT.MLP, gpt2_dims=synth.GPT2_TINY)
    assert isinstance(m.clip_project, gpt2_prefix.MLP) and m.prefix_length == 10 and m.gpt_embedding_size == 768
    m2 = gpt2_prefix.ClipCaptionModel(10, prefix_size=512, gpt2_dims=synth.GPT2_TINY)       # train.py spelling
    assert isinstance(m2.clip_project, transformer_mapper.TransformerMapper) and m2.prefix_dim == 512
    assert train.noise_injection(torch.ones(2, 4), 0.0).equal(torch.ones(2, 4))              # variance 0: identity
    # the image half of the loop: argument checks happen before any device work
    sig = inspect.signature(predictions_runner.make_preds_from_images)
    assert list(sig.parameters)[:6] == ["data", "images", "clip_model", "preprocess", "model", "tokenizer"]
    assert sig.parameters["is_rn"].default is False and sig.parameters["beam"].default is True
    with pytest.raises(ValueError):
        predictions_runner.make_preds_from_images([{"image_id": 1}], [], None, None, None, None)
    with pytest.raises(ValueError):
        predictions_runner.make_preds([{"image_id": 1}], torch.zeros(2, 4), None, None)


def test_timer_matches_the_reference_timer_text():
    """capdec_amd.predictions_runner.Timer prints what the reference's Timer prints (predictions_runner.py:146-149)"""
    from capdec_amd.predictions_runner import Timer
    t = Timer()
    assert str(t) == "mean: nan ms, std: nan ms"
    t.timings, t.sum, t.count = [1.0, 3.0], 4.0, 2
    assert str(t) == "mean: 2.00 ms, std: 1.00 ms"
    t.add_items(8)
    assert str(t).startswith("mean: 2.00 ms, std: 1.00 ms per batch; 0.5000 ms per image over 8 images")


def test_state_dict_loading_rules():
    from capdec_amd import synth
    from capdec_amd.gpt2_prefix import ClipCaptionModel, MappingType
    dims = synth.GPT2_TINY
    sd = synth.hot_state_dict(3, "transformer_encoder", 512, 10, dims=dims)
    m = ClipCaptionModel(10, prefix_dim=512, gpt2_dims=dims)
    # transformers-4.24 checkpoints carry attn.bias / attn.masked_bias buffers: ignored, not rejected
    old = dict(sd)
    old["gpt.transformer.h.0.attn.bias"] = torch.ones(1, 1, 8, 8, dtype=torch.uint8)
    old["gpt.transformer.h.0.attn.masked_bias"] = torch.tensor(-1e4)
    res = m.load_state_dict(old)
    assert not res.unexpected_keys and "gpt.transformer.h.0.attn.bias" not in m.state_dict()
    # fp16 checkpoints are upcast like the reference's .float()
    m.load_state_dict({k: v.half() for k, v in sd.items()})
    assert all(v.dtype == torch.float32 for v in m.state_dict().values())
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("clip_project.")})
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, "bogus.weight": torch.zeros(1)})
    mm = ClipCaptionModel(10, prefix_dim=512, mapping_type=MappingType.MLP, gpt2_dims=dims)
    with pytest.raises(RuntimeError):                                # transformer checkpoint into an MLP model
        mm.load_state_dict(sd)


@pytest.mark.parametrize("variant", ["train_mlp", "eval_transformer"])
def test_loads_checkpoint_written_by_the_reference(tmp_path, variant, golden):
    """Real-artefact readiness without the artefacts: a checkpoint written the way the reference writes it --
    ITS ClipCaptionModel (train.py:246-284 with ``prefix_size`` / gpt2_prefix.py:139-171 with ``prefix_dim``),
    ``torch.save(model.state_dict(), path)`` (train.py:359-371) -- is read back with ``torch.load(map_location=...)``
    (predictions_runner.py:461) and loaded STRICT by ``capdec_amd.gpt2_prefix.ClipCaptionModel``: every tensor the
    reference saved arrives bit for bit, the tied ``gpt.lm_head.weight`` is accepted, and the transformers-4.24 buffers
    (``attn.bias`` / ``attn.masked_bias``; 5.x no longer writes them) are tolerated when present.  The reference's state
    dict is rebuilt from tests/golden/reference_checkpoints.npz (tools/gen_golden.py: every key, shape and dtype the
    reference model's state_dict() holds, and which keys share storage) with seeded values"""
    from collections import OrderedDict
    from capdec_amd import synth
    from capdec_amd import gpt2_prefix as ours
    man = golden("reference_checkpoints")
    dims = synth.GPT2Dims(n_layer=2, vocab=1531, n_pos=128)
    if variant == "train_mlp":
        mine = ours.ClipCaptionModel(10, clip_length=10, prefix_size=512, mapping_type=ours.MappingType.MLP, gpt2_dims=dims)
    else:
        mine = ours.ClipCaptionModel(10, clip_length=10, prefix_dim=640, num_layers=3,
                                     mapping_type=ours.MappingType.TransformerEncoder, gpt2_dims=dims)
    g = torch.Generator().manual_seed(3)
    tied = {str(a): str(b) for a, b in man[f"tied_{variant}"]}
    ref_sd, shapes, at = OrderedDict(), man[f"shapes_{variant}"], 0
    for k, dt, nd in zip(man[f"keys_{variant}"], man[f"dtypes_{variant}"], man[f"ndim_{variant}"]):
        shape = tuple(int(s) for s in shapes[at:at + nd])
        at += int(nd)
        if str(k) in tied:
            ref_sd[str(k)] = ref_sd[tied[str(k)]]                            # one storage, as the reference saves it
        else:
            ref_sd[str(k)] = (torch.randn(shape, generator=g) * 0.02).to(getattr(torch, str(dt)))
    assert at == len(shapes) and tied
    path = str(tmp_path / "coco_prefix_latest.pt")
    torch.save(ref_sd, path)                                                # train.py:359-371
    sd = torch.load(path, map_location=torch.device("cpu"))                 # predictions_runner.py:461
    assert "gpt.lm_head.weight" in sd or "gpt.transformer.wte.weight" in sd
    res = mine.load_state_dict(sd)                                          # strict
    assert res.missing_keys == [] and res.unexpected_keys == []
    got = mine.state_dict()
    for k, v in sd.items():
        assert k in got, k
        assert torch.equal(got[k], v.float()), k
    # the same checkpoint as transformers 4.24 (the reference's pin) wrote it: causal-mask buffers in every block
    sd24 = dict(sd)
    for i in range(dims.n_layer):
        sd24[f"gpt.transformer.h.{i}.attn.bias"] = torch.tril(torch.ones(dims.n_pos, dims.n_pos, dtype=torch.uint8)).view(1, 1, dims.n_pos, dims.n_pos)
        sd24[f"gpt.transformer.h.{i}.attn.masked_bias"] = torch.tensor(-1e4)
    res = mine.load_state_dict(sd24)
    assert res.unexpected_keys == []
    # an fp16 checkpoint (a user's `.half()` export) is upcast; a key the model does not know is refused
    mine.load_state_dict({k: (v.half() if v.is_floating_point() else v) for k, v in sd.items()})
    with pytest.raises(RuntimeError):
        mine.load_state_dict(dict(sd, **{"bridger.0.weight": torch.zeros(2, 2)}))


def test_synth_recipe_is_deterministic():
    from capdec_amd import synth
    a = synth.hot_state_dict(42, "mlp", 640, 10, dims=synth.GPT2_TINY)
    b = synth.hot_state_dict(42, "mlp", 640, 10, dims=synth.GPT2_TINY)
    assert synth.state_dict_checksum(a) == synth.state_dict_checksum(b)
    assert a["gpt.lm_head.weight"] is a["gpt.transformer.wte.weight"]
    assert a["gpt.transformer.h.0.attn.c_attn.weight"].shape == (768, 2304)          # Conv1D [in, out]
    assert a["clip_project.model.0.weight"].shape == (3840, 640)                      # nn.Linear [out, in]
    x = synth.synthetic_clip_embeddings(5, 512, 0)
    np.testing.assert_allclose(x.norm(dim=1).numpy(), 1.0, atol=1e-6)


def test_algorithmic_work_matches_survey():
    sys.path.insert(0, ROOT)
    import bench
    g = bench.algorithmic_flops_per_caption(10, 67, 1, "none")
    b = bench.algorithmic_flops_per_caption(10, 67, 5, "none")
    assert abs(g / 1e9 - 18.19) < 0.05 and abs(b / 1e9 - 83.8) < 0.2
    assert abs(bench.algorithmic_flops_per_caption(10, 12, 1, "none") / 1e9 - 4.50) < 0.02


def test_shard_bounds_cover_exactly():
    from capdec_amd.distributed import shard_bounds, shard_size
    for n in (0, 1, 7, 8, 5000, 5001):
        for w in (1, 2, 3, 4, 8):
            spans = [shard_bounds(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert all(hi - lo <= shard_size(n, w) for lo, hi in spans)


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from capdec_amd import distributed as cd
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{sys.argv[2]}", rank=rank, world_size=world)
N, T = 11, 6                                     # ragged: 11 rows over 2 ranks -> 6 + 5
full = torch.arange(N * 2 * T, dtype=torch.int32).view(N, 2, T)
lens = (torch.arange(N * 2, dtype=torch.int32) % T + 1).view(N, 2)
scores = torch.arange(N * 2, dtype=torch.float32).view(N, 2) * -0.5
lo, hi = cd.shard_bounds(N, rank, world)
g_ids, g_lens, g_sc = cd.gather_ids(full[lo:hi].clone(), lens[lo:hi].clone(), N, scores[lo:hi].clone())
assert torch.equal(g_ids, full) and torch.equal(g_lens, lens) and torch.equal(g_sc, scores), rank
# greedy-shaped ids [n, T] and an empty shard (N < world handled by padding)
g2, l2, _ = cd.gather_ids(full[lo:hi, 0].clone(), lens[lo:hi, 0].clone(), N)
assert torch.equal(g2, full[:, 0]) and torch.equal(l2, lens[:, 0])
lo1, hi1 = cd.shard_bounds(1, rank, world)
g3 = cd.gather_rows(full[lo1:hi1, 0].clone(), 1)
assert torch.equal(g3, full[:1, 0])
cd.check_world(rank, world)
try:
    cd.check_world(rank, world + 1)
    raise SystemExit("check_world accepted a wrong world size")
except RuntimeError:
    pass
dist.destroy_process_group()
print("OK", rank)
"""


def test_gather_ids_gloo_world_size_2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = 29500 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT, str(port)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("OK" in o for o in outs)


_IMG_WORKER = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from capdec_amd import predictions_runner as PR
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{sys.argv[2]}", rank=rank, world_size=world)
# fakes for the device pieces: an "image" is an int, its embedding is [v, v, v, v], its caption ids are [v, v + 1, v + 2]
encoded = []
class Pre:
    def batch(self, imgs): return torch.tensor(imgs, dtype=torch.float32)
class Clip:
    def encode_image(self, px):
        encoded.extend(int(v) for v in px.tolist())
        return px[:, None].repeat(1, 4)
class Model:
    prefix_length = 10
    def parameters(self): yield torch.zeros(0)
def fake_caption_ids(model, emb, stop, beam, beam_size, T, dont_norm, off, rank=0, world=1):
    v = emb[:, 0].to(torch.int32)
    ids = torch.zeros(emb.shape[0], T, dtype=torch.int32)
    ids[:, 0], ids[:, 1], ids[:, 2] = v, v + 1, v + 2
    return ids, torch.full((emb.shape[0],), 3, dtype=torch.int32), None
PR.caption_ids = fake_caption_ids
class Tok:
    def encode(self, s): return [13]
    def decode(self, ids): return " ".join(str(int(i)) for i in ids)
images = [10, None, 30, 40, None, 60, 70]                  # two files the reference would skip (:207-210)
data = [{"image_id": 100 + i} for i in range(len(images))]
out = sys.argv[3]
preds = PR.make_preds_from_images(data, images, Clip(), Pre(), Model(), Tok(), out if rank == 0 else None, beam=True,
                                  entry_length=5, rank=rank, world=world, image_batch=2)
keep = [i for i, im in enumerate(images) if im is not None]
want = [{"caption": f"{images[i]} {images[i] + 1} {images[i] + 2}", "image_id": 100 + i} for i in keep]
assert preds == want, (rank, preds)
# the tower ran on THIS rank's block of the kept images only (5 kept images over 2 ranks: 3 + 2)
lo, hi = (0, 3) if rank == 0 else (3, 5)
assert encoded == [images[i] for i in keep[lo:hi]], (rank, encoded)
if rank == 0:
    assert json.load(open(out)) == want
# more ranks than images: the empty shard still takes part in the gather
one = PR.make_preds_from_images(data[:1], images[:1], Clip(), Pre(), Model(), Tok(), None, entry_length=5, rank=rank, world=world)
assert one == want[:1], (rank, one)
dist.destroy_process_group()
print("OK", rank)
"""


def test_image_driver_shards_the_tower_gloo_world_size_2(tmp_path):
    """round-2 advisor finding: make_preds_from_images ran preprocess + encode_image for ALL images on every rank.  Two
    gloo ranks, fake device pieces: each rank encodes only its block of the kept images, the gathered predictions equal
    the single-process list, skipped files stay skipped, an empty shard still joins the gather"""
    script = tmp_path / "img_worker.py"
    script.write_text(_IMG_WORKER)
    port = 31500 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT, str(port), str(tmp_path / "preds.json")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("OK" in o for o in outs)


_TXT_WORKER = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from capdec_amd import predictions_runner as PR
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{sys.argv[2]}", rank=rank, world_size=world)
# fakes for the device pieces: a caption "c<v>" tokenises to a row starting with v, its embedding is [v, v, v, v], its ids [v, v + 1]
tokenised, encoded = [], []
def tokenize(texts):
    tokenised.extend(texts)
    return torch.tensor([[int(t[1:])] + [0] * 76 for t in texts])
class Clip:
    def encode_text(self, toks):
        encoded.extend(int(v) for v in toks[:, 0].tolist())
        return toks[:, :1].float().repeat(1, 4)
class Model:
    prefix_length = 10
    def parameters(self): yield torch.zeros(0)
def fake_caption_ids(model, emb, stop, beam, beam_size, T, dont_norm, off, rank=0, world=1):
    v = emb[:, 0].to(torch.int32)
    ids = torch.zeros(emb.shape[0], T, dtype=torch.int32)
    ids[:, 0], ids[:, 1] = v, v + 1
    return ids, torch.full((emb.shape[0],), 2, dtype=torch.int32), None
PR.caption_ids = fake_caption_ids
class Tok:
    def encode(self, s): return [13]
    def decode(self, ids): return " ".join(str(int(i)) for i in ids)
data = [{"image_id": 500 + i, "caption": f"c{10 * (i + 1)}"} for i in range(5)]
out = sys.argv[3]
preds = PR.make_preds_from_captions(data, Clip(), Model(), Tok(), tokenize, out if rank == 0 else None, beam=False, entry_length=4,
                                    rank=rank, world=world, text_batch=2)
want = [{"caption": f"{10 * (i + 1)} {10 * (i + 1) + 1}", "image_id": 500 + i} for i in range(5)]
assert preds == want, (rank, preds)
lo, hi = (0, 3) if rank == 0 else (3, 5)                     # 5 captions over 2 ranks: 3 + 2, each tokenised / encoded once
assert tokenised == [d["caption"] for d in data[lo:hi]] and encoded == [10 * (i + 1) for i in range(lo, hi)], (rank, tokenised, encoded)
if rank == 0:
    assert json.load(open(out)) == want
one = PR.make_preds_from_captions(data[:1], Clip(), Model(), Tok(), tokenize, None, beam=False, entry_length=4, rank=rank, world=world)
assert one == want[:1], (rank, one)                          # more ranks than captions: the empty shard joins the gather
dist.destroy_process_group()
print("OK", rank)
"""


def test_text_driver_shards_gloo_world_size_2(tmp_path):
    """make_preds_from_captions (the text-input branch, reference predictions_runner.py:215-218) over two gloo ranks with
    fake device pieces: every rank tokenises / encodes / decodes only its block, the gathered predictions equal the
    single-process list in caption order, rank 0 writes the JSON, an empty shard still joins the gather"""
    script = tmp_path / "txt_worker.py"
    script.write_text(_TXT_WORKER)
    port = 33500 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT, str(port), str(tmp_path / "preds.json")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("OK" in o for o in outs)


def test_shard_consistency_checks():
    """a partial shard without a process group must not be returned as if it were the whole result"""
    from capdec_amd import distributed as cd
    part = torch.zeros(3, 4)
    assert cd.gather_rows(part, 3).shape == (3, 4)            # single process, everything local: fine
    with pytest.raises(RuntimeError):
        cd.gather_rows(part, 5)                               # 3 of 5 rows and nobody to gather from
    cd.check_world(0, 1)
    with pytest.raises(RuntimeError):
        cd.check_world(1, 4)
    # world > N: trailing ranks get EMPTY shards (N = 5 over 4 ranks -> 2, 2, 1, 0)
    assert [cd.shard_bounds(5, r, 4) for r in range(4)] == [(0, 2), (2, 4), (4, 5), (5, 5)]


@pytest.mark.parametrize("n", [2, 8])
def test_bench_spawns_its_own_ranks(n):
    """`python bench.py --gpus N` (the driver's form) must start N ranks itself; --dry-run rehearses the whole N-rank
    control flow on CPU (gloo): sharding, a fake decode, the id gather, barrier + max-over-ranks timing, the per-rank
    table, the comparison with a one-rank pass -- with 2 ranks and with the 8 of a full node"""
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--captions", "5000"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]                        # stdout carries exactly one JSON line
    rec = json.loads(lines[0])
    assert rec["dry_run"] and rec["n_gpus"] == n and rec["ranks"] == list(range(n)) and rec["ids_equal_to_1gpu"]
    per = -(-5000 // n)
    assert [r["captions_per_step"] for r in rec["per_rank"]] == [min(per, max(0, 5000 - r * per)) for r in range(n)]
    assert sum(r["captions_per_step"] for r in rec["per_rank"]) == 5000 and all(r["seconds"] > 0 for r in rec["per_rank"])
    if n == 2:
        # a launcher that started the wrong number of ranks is an error, not a silent mismatch
        bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                             capture_output=True, text=True, timeout=120, env=dict(os.environ, RANK="0", WORLD_SIZE="1"))
        assert bad.returncode != 0 and "WORLD_SIZE=1" in (bad.stderr + bad.stdout)


def test_bench_dump_outputs(tmp_path):
    """`bench.py --dump-outputs DIR` writes what the last timed step returned as DIR/<name>.npy (float32 / float64): the
    same arrays from one rank and from two (the dry run's fake decode), and above the size limit the same seeded sample
    of rows of every array, with the row indices beside them"""
    import bench
    got = {}
    for n in (1, 2):
        d = tmp_path / ("dump%d" % n)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--captions", "300",
                              "--steps", "2", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        got[n] = {f: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got[1]) == ["ids.npy", "lengths.npy", "scores.npy"]
    assert got[1]["ids.npy"].shape == (300, 67) and got[1]["lengths.npy"].shape == (300,)
    for f, a in got[1].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, got[2][f]), f
    ids = torch.arange(1000 * 4, dtype=torch.int64).reshape(1000, 4)
    big = {"ids": ids, "wide": ids[:, :1] + (1 << 30), "scores": torch.linspace(0, 1, 1000)}
    shapes = bench.dump_outputs(str(tmp_path / "s1"), big, limit=8000)
    bench.dump_outputs(str(tmp_path / "s2"), big, limit=8000)
    rows = np.load(tmp_path / "s1" / "rows.npy")
    k = shapes["rows"][0]
    assert 0 < k < 1000 and np.all(np.diff(rows) > 0) and np.array_equal(rows, np.load(tmp_path / "s2" / "rows.npy"))
    assert sum(os.path.getsize(tmp_path / "s1" / (f + ".npy")) - 128 for f in shapes) <= 8000
    w = np.load(tmp_path / "s1" / "wide.npy")
    assert w.dtype == np.float64 and np.array_equal(w[:, 0], rows * 4 + (1 << 30))          # beyond float32: float64
    assert np.array_equal(np.load(tmp_path / "s1" / "ids.npy"), ids.numpy()[rows.astype(np.int64)].astype(np.float32))


def test_bench_watchdog_names_the_phase_a_rank_is_stuck_in():
    """an unattended multi-GPU run must not end silently: a rank that overruns --rank-timeout says where it is and exits 3"""
    code = ("import sys, time; sys.path.insert(0, %r); import bench; w = bench.Watchdog(3, 8, 0.3); w.note('timed region'); "
            "time.sleep(5); print('not reached')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "rank 3 of 8" in out.stderr and "timed region" in out.stderr and "not reached" not in out.stdout


def test_formats_round_trip(tmp_path):
    import pickle
    from capdec_amd import formats, synth
    caps = [{"image_id": 7, "caption": "A dog.", "id": 0}, {"image_id": 9, "caption": "Two cats", "id": 1, "filename": "x.jpg"}]
    txt = synth.synthetic_clip_embeddings(2, 512, seed=1, normalize=False)
    p = tmp_path / "emb.pkl"
    formats.save_embeddings_pickle(str(p), caps, text_embeddings=txt, half=True)        # fp16 like a GPU run
    raw = pickle.load(open(p, "rb"))
    assert set(raw) == {"clip_embedding", "captions", "clip_embedding_text_dave"}
    assert raw["clip_embedding_text_dave"].dtype == torch.float16 and raw["captions"][1]["clip_embedding"] == 1
    img, t2, c2 = formats.load_embeddings_pickle(str(p))
    assert img.shape == (0, 512) and t2.dtype == torch.float32 and t2.shape == (2, 512)
    np.testing.assert_allclose(t2.numpy(), txt.half().float().numpy())
    assert c2[0]["caption"] == "A dog."
    # image-only pickle exactly as the reference writes it when add_text_embedding is False
    # (embeddings_generator.py:101: 'clip_embedding_text_dave': 0 -- an int, not a tensor) and the text-only mirror
    # (empty image tensor)
    imgs = synth.synthetic_clip_embeddings(3, 640, seed=2, normalize=False)
    q0 = tmp_path / "img_only.pkl"
    pickle.dump({"clip_embedding": imgs.half(), "captions": caps, "clip_embedding_text_dave": 0}, open(q0, "wb"))
    i3, t3, _ = formats.load_embeddings_pickle(str(q0))
    assert i3.shape == (3, 640) and t3.shape == (0, 640) and i3.dtype == torch.float32
    pickle.dump({"clip_embedding": torch.tensor([]), "captions": caps, "clip_embedding_text_dave": txt}, open(q0, "wb"))
    i4, t4, _ = formats.load_embeddings_pickle(str(q0))
    assert i4.shape == (0, 512) and t4.shape == (2, 512)
    pickle.dump({"clip_embedding": torch.tensor(0), "captions": [], "clip_embedding_text_dave": None}, open(q0, "wb"))
    i5, t5, _ = formats.load_embeddings_pickle(str(q0))
    assert i5.shape[0] == 0 and t5.shape[0] == 0
    # the reference's real modality-offset pickle layout
    off = {k: torch.randn(1, 640) for k in ("center_text", "center_image", "offset_to_add_in_training", "offset_to_add_in_inference")}
    q = tmp_path / "centers.pkl"
    pickle.dump(off, open(q, "wb"))
    o = formats.load_modality_offset(str(q))
    assert o.shape == (1, 640) and torch.equal(o, off["offset_to_add_in_inference"])
    with pytest.raises(KeyError):
        formats.load_modality_offset(str(q), "nope")
    sd = synth.hot_mlp_mapper_state_dict(1, 512, 10)
    ck = tmp_path / "m.pt"
    torch.save(sd, ck)
    assert set(formats.load_checkpoint(str(ck))) == set(sd)
    torch.save({"state_dict": sd, "epoch": 3}, ck)
    assert set(formats.load_checkpoint(str(ck))) == set(sd)
    js = formats.write_predictions_json(str(tmp_path / "p.json"), ["A Dog.", "CATS"], [7, 9])
    assert js == [{"caption": "a dog.", "image_id": 7}, {"caption": "cats", "image_id": 9}]


def _toy_bpe(corpus_words, n_merges, end_of_word=""):
    """tiny BPE trainer (test helper): returns the ranked merge list over byte-unicode symbols"""
    from collections import Counter
    from capdec_amd.bpe import bytes_to_unicode
    be = bytes_to_unicode()
    words = Counter()
    for w in corpus_words:
        sym = [be[b] for b in w.encode("utf-8")]
        if end_of_word:
            sym[-1] = sym[-1] + end_of_word
        words[tuple(sym)] += 1
    merges = []
    for _ in range(n_merges):
        pairs = Counter()
        for w, c in words.items():
            for a, b in zip(w[:-1], w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = max(sorted(pairs), key=lambda p: pairs[p])
        merges.append(best)
        new = Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i < len(w) - 1 and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1]); i += 2
                else:
                    out.append(w[i]); i += 1
            new[tuple(out)] += c
        words = new
    return merges


_TEXTS = ["A man riding a wave on top of a surfboard.", "two dogs' bowls aren't here,  I'll say!!", "  naïve café déjà-vu ☕ 123 4567",
          "the the the cat sat on the mat", "don't you've we're he'd", "x", "Ünïcödé and tabs\tand\nnewlines  "]


def test_gpt2_bpe_matches_transformers(tmp_path):
    import json
    from transformers import GPT2Tokenizer
    from capdec_amd.bpe import GPT2BPE, bytes_to_unicode
    corpus = " ".join(_TEXTS).replace("\t", " ").split(" ")
    corpus = [w for w in corpus if w] + [" " + w for w in corpus if w]
    merges = _toy_bpe(corpus, 120)
    vocab = {c: i for i, c in enumerate(bytes_to_unicode().values())}
    for a, b in merges:
        vocab.setdefault(a + b, len(vocab))
    vf, mf = tmp_path / "vocab.json", tmp_path / "merges.txt"
    vf.write_text(json.dumps(vocab), encoding="utf-8")
    mf.write_text("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n", encoding="utf-8")
    ref = GPT2Tokenizer(vocab=str(vf), merges=str(mf))          # transformers >= 5 signature
    mine = GPT2BPE(str(vf), str(mf))
    for t in _TEXTS:
        ids = mine.encode(t)
        assert ids == ref.encode(t), t
        assert mine.decode(ids, clean_up_tokenization_spaces=False) == t      # byte-level BPE is lossless
        assert mine.decode(ids, clean_up_tokenization_spaces=False) == ref.decode(ids, clean_up_tokenization_spaces=False)
        # the reference calls tokenizer.decode(ids) under transformers 4.24, whose default cleans up " ." " ," " n't" ...
        # (transformers >= 5 ignores the flag for BPE tokenizers, so apply its clean_up_tokenization explicitly = 4.24's decode)
        assert mine.decode(ids) == ref.clean_up_tokenization(ref.decode(ids, clean_up_tokenization_spaces=False))
    cap = "a man , who isn't here , rides a wave 's crest . really ? yes ! we 're sure , i 'm ' fine ' and they 've gone ."
    assert GPT2BPE.clean_up_tokenization(cap) == ref.clean_up_tokenization(cap) \
        == "a man, who isn't here, rides a wave's crest. really? yes! we're sure, i'm'fine'and they've gone."
    assert mine.encode(".")[0] == ref.encode(".")[0]        # the stop-token lookup the decode functions do


def test_clip_bpe_matches_transformers(tmp_path):
    import json
    from transformers import CLIPTokenizer
    from capdec_amd.bpe import ClipBPE
    words = [w.lower() for t in _TEXTS for w in t.replace("\t", " ").split() if w]
    merges = _toy_bpe(words, 150, end_of_word="</w>")
    mine = ClipBPE(merges)
    vf, mf = tmp_path / "vocab.json", tmp_path / "merges.txt"
    vf.write_text(json.dumps(mine.encoder), encoding="utf-8")
    mf.write_text("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n", encoding="utf-8")
    ref = CLIPTokenizer(vocab=str(vf), merges=str(mf))
    ascii_texts = [t for t in _TEXTS if t.isascii()]          # non-ascii cleaning differs without ftfy (both sides lack it here)
    for t in ascii_texts:
        want = ref(t)["input_ids"]
        got = [mine.sot] + mine.encode(t) + [mine.eot]
        assert got == want, t
    rows = mine.tokenize(ascii_texts)
    assert rows.shape == (len(ascii_texts), 77) and rows.dtype == torch.int32
    assert (rows[:, 0] == mine.sot).all() and all(int(r.max()) == mine.eot for r in rows)
    assert int(rows[0].argmax()) == len(mine.encode(ascii_texts[0])) + 1         # EOT position = argmax (encode_text pooling)
    with pytest.raises(RuntimeError):
        mine.tokenize("word " * 100)
    assert mine.tokenize("word " * 100, truncate=True)[0, 76] == mine.eot


def test_pmc_summary_tool(tmp_path):
    """tools/pmc_summary.py: per-kernel averages of the two rocprofv3 --pmc passes and the gfx950 FETCH_SIZE correction
    (traffic = 2 x FETCH_SIZE + WRITE_SIZE, counters in KB)"""
    import json
    d = tmp_path / "pmc_FETCH_SIZE" / "box"
    d.mkdir(parents=True)
    (d / "1_counter_collection.csv").write_text(
        '"Kernel_Name","Counter_Name","Counter_Value"\n'
        '"void capdec::gemm_bf16x3p_kernel<true>(int, float*)","FETCH_SIZE",1000\n'
        '"void capdec::gemm_bf16x3p_kernel<true>(int, float*)","FETCH_SIZE",3000\n'
        '"capdec::layernorm_packed_kernel(float const*)","FETCH_SIZE",10\n')
    d2 = tmp_path / "pmc_WRITE_SIZE" / "box"
    d2.mkdir(parents=True)
    (d2 / "2_counter_collection.csv").write_text(
        '"Kernel_Name","Counter_Name","Counter_Value"\n'
        '"void capdec::gemm_bf16x3p_kernel<true>(int, float*)","WRITE_SIZE",500\n'
        '"void capdec::gemm_bf16x3p_kernel<true>(int, float*)","WRITE_SIZE",700\n')
    out = tmp_path / "traffic.json"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "pmc_summary.py"), str(tmp_path), str(out), "cmd"])
    rec = json.load(open(out))
    k = rec["kernels"]["gemm_bf16x3p_kernel<true>"]
    assert k["launches"] == 2 and k["fetch_KB_raw"] == 2000.0 and k["write_KB"] == 600.0
    assert k["traffic_bytes_per_launch"] == (2 * 2000 + 600) * 1024
    assert rec["gemm_bf16x3p_kernel"] == k                       # alias without template arguments (what bench.py reads)
    assert rec["kernels"]["layernorm_packed_kernel"]["traffic_bytes_per_launch"] == 20 * 1024


def test_dropout_stream_layout_matches_the_oracle_call_order():
    """the mask stream capdec_train_set_dropout_masks expects (Engine.dropout_stream_size; include/capdec.h) is the
    oracle's dropout_sites -- transformers' GPT2Model call order -- flattened: same total, embd first, then per block
    attn [B, H, S, S], resid, mlp"""
    import numpy as np
    from capdec_amd.engine import Engine
    from oracle import capdec_oracle as O
    for (L, B, S, d, H) in [(2, 4, 19, 768, 12), (12, 34, 60, 768, 12), (1, 1, 11, 768, 12)]:
        sites = O.dropout_sites(L, B, S, d, H)
        assert Engine.dropout_stream_size(B, S, d, H, L) == sum(int(np.prod(sh)) for _, sh in sites)
        assert [n for n, _ in sites][:4] == ["embd", "h.0.attn", "h.0.resid", "h.0.mlp"]
        assert sites[1][1] == (B, H, S, S) and sites[0][1] == sites[2][1] == sites[3][1] == (B, S, d)


def test_train_loop_control_flow_with_fake_device(tmp_path, monkeypatch):
    """capdec_amd.train.train (reference train.py:317-392) on CPU with the device pieces faked: epochs x batches of a
    drop_last DataLoader, scheduler stepped after every batch, steps enqueued (wait=False) and the epoch mean taken from the
    engine's running sum, checkpoints `{prefix}-{epoch:03d}.pt` at save_every and at the last epoch, the validation pass once
    per epoch when a validation dataset is given, `loss_per_epoch.json` = {'train': [...], 'val': [...]} rewritten every
    epoch, and args.val_pt without a dataset refused"""
    import json
    from types import SimpleNamespace
    from capdec_amd import train as Tr
    from capdec_amd._capi import CapdecError
    calls = {"steps": [], "lrs": [], "val": 0}

    class FakeEngine:
        def __init__(self):
            self.sum, self.n = 0.0, 0

        def train_loss(self, reset=False):
            out = (0.0, self.sum, self.n)
            if reset:
                self.sum, self.n = 0.0, 0
            return out

    class FakeModel:
        prefix_length = 10

        def __init__(self):
            self.engine, self.training = FakeEngine(), False

        def train(self, mode=True):
            self.training = mode
            return self

        def parameters(self):
            return iter(())

        def state_dict(self):
            return {"clip_project.w": torch.zeros(1)}

    def fake_train_step(model, optimizer, tokens, mask, prefix, *, apply_update=True, dropout_masks=None, wait=True):
        assert wait is False and model.training
        calls["steps"].append(tokens.shape[0])
        calls["lrs"].append(optimizer.param_groups[0]["lr"])
        model.engine.sum += 2.0 + 0.5 * len(calls["steps"])
        model.engine.n += 1

    def fake_validation_loss(model, ds, bs, P=None):
        calls["val"] += 1
        return 7.0 + calls["val"]

    monkeypatch.setattr(Tr, "train_step", fake_train_step)
    monkeypatch.setattr(Tr, "validation_loss", fake_validation_loss)
    monkeypatch.setattr(Tr, "noise_injection", lambda x, *a, **k: x)
    monkeypatch.setattr(Tr, "device", torch.device("cpu"))
    ds = [(torch.ones(5, dtype=torch.int64), torch.ones(15), torch.zeros(512)) for _ in range(10)]     # bs 4 -> 2 batches (drop_last)
    args = SimpleNamespace(bs=4, epochs=3, lr=1e-3, noise_variance=0.016, uniform_noise=False, dont_norm=False, save_every=2, val_pt="")
    model = FakeModel()
    Tr.train(ds, model, args, warmup_steps=2, output_dir=str(tmp_path), output_prefix="run", val_dataset=ds[:4])
    assert calls["steps"] == [4] * 6 and calls["val"] == 3
    assert calls["lrs"][0] == 0.0 and abs(calls["lrs"][2] - 1e-3) < 1e-12 and calls["lrs"][3] < 1e-3      # warm-up, then linear decay
    rec = json.load(open(tmp_path / "loss_per_epoch.json"))
    assert rec["val"] == [8.0, 9.0, 10.0]
    np.testing.assert_allclose(rec["train"], [(2.5 + 3.0) / 2, (3.5 + 4.0) / 2, (4.5 + 5.0) / 2])
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pt")) == ["run-000.pt", "run-002.pt"]
    with pytest.raises(CapdecError):
        Tr.train(ds, model, SimpleNamespace(**dict(vars(args), val_pt="val.pkl")), output_dir=str(tmp_path))


def test_train_step_facade_scope_and_dropout_decisions_without_a_device():
    """capdec_amd.train.train_step up to the first device transfer, with a recording fake engine: a ClipCaptionPrefix asks for
    scope 0 and never touches the dropout setting; a plain ClipCaptionModel asks for scope 1 and -- in train() mode -- for
    model.gpt.config.resid_pdrop (0.1) exactly once, for 0 after eval(); injected masks need dropout to be on; host-side token
    ids outside the vocabulary raise IndexError before anything reaches the device (the reference's embedding lookup)"""
    from capdec_amd import train as Tr, synth
    from capdec_amd._capi import CapdecError
    from capdec_amd.gpt2_prefix import ClipCaptionModel, ClipCaptionPrefix, MappingType

    class Rec:
        def __init__(self):
            self.calls = []

        def train_set_scope(self, full):
            self.calls.append(("scope", bool(full)))

        def train_set_dropout(self, p, seed):
            self.calls.append(("dropout", round(float(p), 6)))

        def train_set_dropout_masks(self, m):
            self.calls.append(("masks", int(m.numel())))

    def make(cls):
        m = cls(10, clip_length=10, prefix_size=512, num_layers=8, mapping_type=MappingType.MLP, gpt2_dims=synth.GPT2_TINY)
        m._engine = Rec()
        m._dirty = False
        return m

    tokens = torch.randint(1, synth.GPT2_TINY.vocab, (2, 5))
    prefix = torch.zeros(2, 512)
    opt = Tr.AdamW(None, lr=1e-3)

    def run(model, **kw):
        try:
            Tr.train_step(model, opt, tokens, None, prefix, **kw)
        except (IndexError, CapdecError):
            raise
        except Exception:
            pass                                  # (no GPU here: the transfer of `tokens` is where the CPU run ends)
        return model._engine.calls

    pre = make(ClipCaptionPrefix)
    if not hasattr(type(pre), "engine") or not isinstance(getattr(type(pre), "engine", None), property):
        pytest.skip("engine is not a property on this build of the facade")
    pre.train()
    assert run(pre) == [("scope", False)]
    full = make(ClipCaptionModel)
    full.train()
    assert run(full) == [("scope", True), ("dropout", 0.1)]
    assert run(full) == [("scope", True), ("dropout", 0.1), ("scope", True)]            # same setting: not re-seeded
    full.eval()
    assert run(full)[-2:] == [("scope", True), ("dropout", 0.0)]
    with pytest.raises(CapdecError):
        run(full, dropout_masks=torch.ones(8, dtype=torch.uint8))                       # eval mode: no dropout to inject into
    full.train()
    assert ("masks", 8) in run(full, dropout_masks=torch.ones(8, dtype=torch.uint8))
    # a NEW context (model.to(other device), use_measurement_build: the engine object is replaced) starts at p = 0 on the
    # device: the same (p, epoch) must be set up again, or full-scope training would silently run without dropout
    full._engine = Rec()
    assert run(full) == [("scope", True), ("dropout", 0.1)]
    bad = tokens.clone()
    bad[0, 0] = synth.GPT2_TINY.vocab
    with pytest.raises(IndexError):
        Tr.train_step(full, opt, bad, None, prefix)


def test_stop_bias_variant_of_the_synthetic_weights_ends_captions():
    """synth.with_stop_bias (bench.py's stop profile, the headline-size stop test): only the stop row changes, the tied
    lm_head follows, the stop token's logit rises by ~alpha at every position, and under the oracle's greedy decode the
    captions of the tiny geometry end (they never do on the unmodified weights, whose stop id is never emitted)"""
    from oracle import capdec_oracle as O
    dims = synth.GPT2_TINY
    sd0 = synth.hot_state_dict(42, "mlp", 512, 10, dims=dims)
    sd1 = synth.with_stop_bias(sd0, 13, 20.0)
    w0, w1 = sd0["gpt.transformer.wte.weight"], sd1["gpt.transformer.wte.weight"]
    assert sd1["gpt.lm_head.weight"] is w1 and torch.equal(w0[:13], w1[:13]) and torch.equal(w0[14:], w1[14:])
    b = sd0["gpt.transformer.ln_f.bias"]
    assert abs(float((w1[13] - w0[13]) @ b) - 20.0) < 1e-3
    assert all(sd1[k] is sd0[k] for k in sd0 if k not in ("gpt.transformer.wte.weight", "gpt.lm_head.weight"))
    x = synth.synthetic_clip_embeddings(6, 512, seed=0)
    pe = O.clip_project(O.normalize_prefix(x), sd0, "mlp", 10)
    d = O.gpt2_logits(pe, sd1, dims.n_head)[:, :, 13] - O.gpt2_logits(pe, sd0, dims.n_head)[:, :, 13]
    assert 10.0 < float(d.mean()) < 30.0 and float(d.min()) > 0.0
    _, l0 = O.greedy_cached(sd0, pe, stop_id=13, entry_length=24, alt_stop_id=-1, n_head=dims.n_head)
    assert int(l0.min()) == 24
    lens = None
    for alpha in (8.0, 16.0, 32.0, 64.0, 128.0):          # (the offset that ends captions depends on the geometry's logit scale)
        _, lens = O.greedy_cached(synth.with_stop_bias(sd0, 13, alpha), pe, stop_id=13, entry_length=24, alt_stop_id=-1, n_head=dims.n_head)
        if float(lens.float().mean()) < 12.0:
            break
    assert float(lens.float().mean()) < 12.0
