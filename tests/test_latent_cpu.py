"""Host side of latent-space rendering (rgb_as_latents) — no GPU needed: the VAE decoder's parameter layout against the reference
Decoder's own names (recorded in the fixtures by tests/golden/make_goldens_latent.py), the diffusers name mapping, the checkpoint
round trip, the packed weight table against the one asd_vae_dec_* publishes, its workspace query, and the guidance's argument and
draw-order contract in latent mode."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR


def _golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


@pytest.mark.parametrize("fixture,ch", [("diffusion_vae_decoder_full_64", 128), ("diffusion_vae_decoder_small", 32)])
def test_decoder_layout_has_the_reference_names_and_shapes(fixture, ch):
    from scaledreamer_amd.diffusion import weights as W

    g = _golden(fixture)
    cfg = W.VAEConfig(ch=ch)
    assert int(g["cfg"][0]) == ch and tuple(g["ch_mult"]) == cfg.ch_mult
    ref = {str(n): tuple(int(d) for d in str(s).split(",")) for n, s in zip(g["names"], g["name_shapes"])}
    shapes, plan = W.vae_decoder_layout(cfg)
    assert {k: tuple(v) for k, v in shapes.items()} == ref
    # num_res_blocks + 1 blocks per level, a shortcut exactly where the width changes, an upsampler on every level but 0
    for lvl in range(len(cfg.ch_mult)):
        assert f"decoder.up.{lvl}.block.{cfg.num_res_blocks}.conv1.weight" in shapes and f"decoder.up.{lvl}.block.{cfg.num_res_blocks + 1}.conv1.weight" not in shapes
        assert (f"decoder.up.{lvl}.upsample.conv.weight" in shapes) == (lvl > 0)
    for kind, name, cin, cout in plan:
        if kind == "res":
            assert (name + ".nin_shortcut.weight" in shapes) == (cin != cout)
    assert [k for k, *_ in plan][:6] == ["post_quant", "conv", "res", "attn", "res", "res"] and plan[-1][0] == "out"


def _diffusers_vae_decoder_names(cfg):
    """parameter names of the decoder half of diffusers' AutoencoderKL (UNetMidBlock2D with one attention, UpDecoderBlock2D x n_levels
    in execution order, each with num_res_blocks + 1 resnets), written out from the architecture — not from our mapping."""
    names = []

    def add(prefix, leaves):
        for l in leaves:
            names.extend([f"{prefix}.{l}.weight", f"{prefix}.{l}.bias"])

    res = ["norm1", "conv1", "norm2", "conv2"]
    add("decoder", ["conv_in", "conv_norm_out", "conv_out"])
    names.extend(["post_quant_conv.weight", "post_quant_conv.bias"])
    add("decoder.mid_block.resnets.0", res)
    add("decoder.mid_block.resnets.1", res)
    add("decoder.mid_block.attentions.0", ["group_norm", "to_q", "to_k", "to_v", "to_out.0"])
    n = len(cfg.ch_mult)
    widths = [cfg.ch * m for m in reversed(cfg.ch_mult)]          # execution order: the deepest level first
    cin = widths[0]
    for i, cout in enumerate(widths):
        for j in range(cfg.num_res_blocks + 1):
            add(f"decoder.up_blocks.{i}.resnets.{j}", res + (["conv_shortcut"] if cin != cout else []))
            cin = cout
        if i != n - 1:
            add(f"decoder.up_blocks.{i}.upsamplers.0", ["conv"])
    return names


def test_diffusers_decoder_names_map_one_to_one_onto_the_layout():
    from scaledreamer_amd.diffusion import checkpoint as CK, weights as W

    for cfg in (W.VAEConfig(), W.VAEConfig(ch=32)):
        shapes, _ = W.vae_decoder_layout(cfg)
        names = _diffusers_vae_decoder_names(cfg)
        mapped = [CK.diffusers_vae_decoder_key_to_ldm(k, cfg) for k in names]
        assert None not in mapped and len(set(mapped)) == len(mapped) and set(mapped) == set(shapes)
    full = W.VAEConfig()
    assert CK.diffusers_vae_decoder_key_to_ldm("decoder.up_blocks.0.resnets.2.conv1.weight", full) == "decoder.up.3.block.2.conv1.weight"
    assert CK.diffusers_vae_decoder_key_to_ldm("decoder.up_blocks.2.resnets.0.conv_shortcut.bias", full) == "decoder.up.1.block.0.nin_shortcut.bias"
    assert CK.diffusers_vae_decoder_key_to_ldm("decoder.up_blocks.2.upsamplers.0.conv.weight", full) == "decoder.up.1.upsample.conv.weight"
    assert CK.diffusers_vae_decoder_key_to_ldm("decoder.mid_block.attentions.0.to_out.0.weight", full) == "decoder.mid.attn_1.proj_out.weight"
    assert CK.diffusers_vae_decoder_key_to_ldm("decoder.mid_block.attentions.0.query.bias", full) == "decoder.mid.attn_1.q.bias"
    assert CK.diffusers_vae_decoder_key_to_ldm("decoder.conv_norm_out.weight", full) == "decoder.norm_out.weight"
    # the encoder half is none of its business, and the encoder's mapping still ignores the decoder
    assert CK.diffusers_vae_decoder_key_to_ldm("encoder.conv_in.weight", full) is None and CK.diffusers_vae_decoder_key_to_ldm("quant_conv.bias", full) is None
    assert CK.diffusers_vae_key_to_ldm("decoder.conv_in.weight") is None and CK.diffusers_vae_key_to_ldm("post_quant_conv.weight") is None
    with pytest.raises(KeyError):
        CK.diffusers_vae_decoder_key_to_ldm("decoder.up_blocks.0.attentions.0.to_q.weight", full)


def test_resolve_decoder_params_round_trips_both_checkpoint_formats(tmp_path):
    from types import SimpleNamespace

    from scaledreamer_amd.diffusion import checkpoint as CK, weights as W

    cfg = W.VAEConfig(ch=32)
    shapes, _ = W.vae_decoder_layout(cfg)
    dp = W.gen_params(shapes, 9)
    ep = W.gen_params(W.vae_encoder_layout(cfg)[0], 6)
    ldm = {"first_stage_model." + k: v for k, v in {**dp, **ep}.items()}
    ldm["model.diffusion_model.time_embed.0.weight"] = torch.zeros(1)            # not the decoder's: ignored
    torch.save({"state_dict": ldm}, tmp_path / "mv.pt")
    got, what = CK.resolve_decoder_params(SimpleNamespace(ckpt_path=str(tmp_path / "mv.pt")), cfg)
    assert "LDM checkpoint" in what and set(got) == set(shapes) and all(torch.equal(got[k], dp[k]) for k in shapes)
    got, what = CK.resolve_decoder_params(SimpleNamespace(pretrained_model_name_or_path=str(tmp_path / "mv.pt")), cfg)
    assert all(torch.equal(got[k], dp[k]) for k in shapes)

    inv = {CK.diffusers_vae_decoder_key_to_ldm(k, cfg): k for k in _diffusers_vae_decoder_names(cfg)}
    (tmp_path / "sd" / "vae").mkdir(parents=True)
    vae = {inv[k]: v for k, v in dp.items()}
    for k in ("decoder.mid_block.attentions.0.to_q.weight", "decoder.mid_block.attentions.0.to_out.0.weight"):
        vae[k] = vae[k].reshape(vae[k].shape[:2])                                  # newer diffusers store these 1x1 convolutions as Linear
    vae["encoder.conv_in.weight"] = torch.zeros(1)                                # the encoder half: ignored here
    vae["quant_conv.weight"] = torch.zeros(1)
    torch.save(vae, tmp_path / "sd" / "vae" / "diffusion_pytorch_model.bin")
    got, what = CK.resolve_decoder_params(SimpleNamespace(pretrained_model_name_or_path=str(tmp_path / "sd")), cfg)
    assert "diffusers pipeline" in what and set(got) == set(shapes)
    assert all(tuple(got[k].shape) == tuple(shapes[k]) and torch.equal(got[k].reshape(-1), dp[k].reshape(-1)) for k in shapes)

    broken = dict(vae)
    del broken["decoder.conv_out.bias"]
    torch.save(broken, tmp_path / "sd" / "vae" / "diffusion_pytorch_model.bin")
    with pytest.raises(KeyError, match="missing"):
        CK.resolve_decoder_params(SimpleNamespace(pretrained_model_name_or_path=str(tmp_path / "sd")), cfg)
    # nothing on disk: an error, and seeded random weights (None) only behind allow_random_weights
    with pytest.raises(CK.MissingWeightsError):
        CK.resolve_decoder_params(SimpleNamespace(pretrained_model_name_or_path=str(tmp_path / "nowhere")), cfg)
    got, what = CK.resolve_decoder_params(SimpleNamespace(pretrained_model_name_or_path=str(tmp_path / "nowhere"), allow_random_weights=True,
                                                          weights_seed=3), cfg)
    assert got is None and "seed 3" in what
    # resolve_params keeps its three-part result and keeps ignoring the decoder's tensors
    up = W.gen_params(W.unet_layout(W.UNetConfig(model_channels=32, num_head_channels=32, context_dim=16))[0], 5)
    torch.save({"state_dict": {**ldm, **{"model.diffusion_model." + k: v for k, v in up.items()}}}, tmp_path / "all.pt")
    u, v, what = CK.resolve_params(SimpleNamespace(ckpt_path=str(tmp_path / "all.pt")), W.UNetConfig(model_channels=32, num_head_channels=32, context_dim=16), cfg)
    assert set(v) == set(W.vae_encoder_layout(cfg)[0]) and set(u) == set(up)


def _dec_table(cfg):
    from scaledreamer_amd._lib import WeightInfo, check, i32, lib
    from scaledreamer_amd.diffusion.vae_hip import vae_desc

    h = C.c_void_p()
    check(lib().asd_vae_dec_create(C.byref(vae_desc(cfg)), C.byref(h)))
    info, out = WeightInfo(), {}
    for i in range(lib().asd_vae_dec_num_weights(h)):
        check(lib().asd_vae_dec_weight_info(h, i32(i), C.byref(info)))
        out[info.name.decode()] = (info.rows, info.cols)
    assert lib().asd_vae_dec_weight_info(h, i32(len(out)), C.byref(info)) != 0       # out of range -> error status
    return h, out


def test_decoder_weight_table_matches_the_packer():
    from scaledreamer_amd._lib import lib
    from scaledreamer_amd.diffusion import weights as W

    for cfg in (W.VAEConfig(), W.VAEConfig(ch=32)):
        h, t = _dec_table(cfg)
        p = W.gen_params(W.vae_decoder_layout(cfg)[0], 3) if cfg.ch == 32 else {k: torch.zeros(v) for k, v in W.vae_decoder_layout(cfg)[0].items()}
        packed = W.pack_vae_decoder(p, cfg)
        assert list(t) and set(t) == set(packed)
        for k, (r, c) in t.items():
            assert packed[k].numel() == r * c, (k, tuple(packed[k].shape), r, c)
        assert not any(k.endswith((".bwd", ".wt")) for k in t) and not any("post_quant" in k for k in t)       # forward only; prep kernel's
        top = cfg.ch * cfg.ch_mult[-1]
        assert t["decoder.conv_in.fwd"] == (top, 9 * 32) and t["decoder.conv_out.fwd"] == (32, 9 * cfg.ch) and t["decoder.conv_out.bias"] == (1, 32)
        c1 = cfg.ch * cfg.ch_mult[1]
        assert t["decoder.up.1.upsample.conv.fwd"] == (4 * c1, 4 * c1)                # parity form
        if cfg.ch == 32:
            # conv_out: rows 3..31 and their biases are zero padding; the parity form sums the taps that land on one low-resolution pixel
            wo = packed["decoder.conv_out.fwd"]
            assert float(wo[3:].abs().max()) == 0.0 and float(packed["decoder.conv_out.bias"][3:].abs().max()) == 0.0
            assert torch.equal(wo[:3].reshape(3, 3, 3, cfg.ch), p["decoder.conv_out.weight"].permute(0, 2, 3, 1))
            wu = packed["decoder.up.1.upsample.conv.fwd"].reshape(2, 2, c1, 2, 2, c1)
            w = p["decoder.up.1.upsample.conv.weight"]
            torch.testing.assert_close(wu[0, 1, :, 1, 0], w[:, :, 1, 0] + w[:, :, 1, 1] + w[:, :, 2, 0] + w[:, :, 2, 1])
            pq = W.post_quant_matrix(p)
            assert pq.shape == (20,) and torch.equal(pq[:16].reshape(4, 4), p["post_quant_conv.weight"].reshape(4, 4)) and torch.equal(pq[16:], p["post_quant_conv.bias"])
        lib().asd_vae_dec_destroy(h)


def test_decoder_workspace_query_needs_no_device_and_rejects_bad_sizes():
    from scaledreamer_amd._lib import i32, lib
    from scaledreamer_amd.diffusion import weights as W

    ASD_ERR_ARG = 1
    l = lib()
    h, _ = _dec_table(W.VAEConfig())
    sizes = [l.asd_vae_dec_workspace_bytes(h, i32(b), i32(64), i32(64), i32(0)) for b in (1, 2, 4)]
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    act = 512 * 512 * 256 * 2              # the widest activation: the upsampled 256-channel tensor entering level 0
    assert 4 * act <= sizes[0] < 6 * act and sizes[2] - sizes[1] >= 2 * 4 * act        # four rotating buffers dominate; nothing per layer
    assert l.asd_vae_dec_workspace_bytes(h, i32(1), i32(64), i32(64), i32(1)) == sizes[0]     # fixed tiles: nothing to tune, no tuning scratch
    for b, hl, wl in [(0, 64, 64), (17, 8, 8), (1, 0, 64), (1, 64, 0), (1, 7, 8), (1, 8, 7), (1, -2, 8), (1, 6, 6)]:
        assert l.asd_vae_dec_workspace_bytes(h, i32(b), i32(hl), i32(wl), i32(0)) == -ASD_ERR_ARG, (b, hl, wl)
        assert b"VAE decoder" in l.asd_last_error()
    assert l.asd_vae_dec_workspace_bytes(None, i32(1), i32(64), i32(64), i32(0)) == -ASD_ERR_ARG
    small, _ = _dec_table(W.VAEConfig(ch=32))
    assert 0 < l.asd_vae_dec_workspace_bytes(small, i32(2), i32(8), i32(8), i32(0)) < sizes[0]
    assert l.asd_vae_dec_workspace_bytes(small, i32(1), i32(6), i32(4), i32(0)) > 0           # even sides, 24 positions
    l.asd_vae_dec_destroy(h)
    l.asd_vae_dec_destroy(small)


def _guidances():
    from scaledreamer_amd.guidance import (DiffusionBackend, MVDreamTimestepShiftedScoreDistillationGuidance as MV, PromptUtils,
                                           SDTimestepShiftedScoreDistillationGuidance as SD)

    be = DiffusionBackend()
    be.device = "cpu"
    pu = PromptUtils.synthetic(seed=1)
    return SD({"guidance_perp_neg": -0.5}, backend=be), MV({}, backend=be), pu


def test_rgb_as_latents_with_three_channels_is_a_value_error():
    sd, mv, pu = _guidances()
    cam = (torch.zeros(4), torch.zeros(4), torch.ones(4))
    rgb3 = torch.rand(4, 8, 8, 3)
    with pytest.raises(ValueError, match="3 channels"):
        sd(rgb3, pu, *cam, rgb_as_latents=True)
    with pytest.raises(ValueError, match="3 channels"):
        mv(rgb3, pu, *cam, torch.eye(4).repeat(4, 1, 1), rgb_as_latents=True)
    with pytest.raises(ValueError, match="3 channels"):
        sd.decode_latents(torch.rand(1, 3, 8, 8))
    assert not hasattr(mv, "decode_latents")                  # the reference's MVDream guidance has none


class _OnDevice(torch.Tensor):
    """a host tensor that answers is_cuda: lets _distill's draw logic run here, up to the node that would launch kernels"""

    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize("which", ["sd", "mv"])
def test_latent_mode_draws_only_the_noise(which, monkeypatch):
    """the reference draws `noise`, `t` and the t+ uniforms in latent mode and nothing for a posterior: the draw order is the contract"""
    from scaledreamer_amd import guidance as G

    sd, mv, pu = _guidances()
    guid = sd if which == "sd" else mv
    order, jobs = [], []

    def no_posterior(like):
        raise AssertionError("latent mode drew a posterior sample")

    def noise(like):
        order.append("noise")
        return torch.zeros_like(like)

    def timesteps(lo, hi, n, device):
        order.append("t")
        return torch.full((n,), 500, dtype=torch.long)

    guid.posterior_noise_fn, guid.noise_fn, guid.timestep_fn = no_posterior, noise, timesteps

    class Node:
        @staticmethod
        def apply(rgb, backend, job):
            jobs.append(job)
            return torch.zeros(()), torch.zeros(())
    monkeypatch.setattr(G, "_ScoreDistillation", Node)
    render = torch.zeros(4, 8, 8, 4).as_subclass(_OnDevice)
    cam = (torch.zeros(4), torch.zeros(4), torch.ones(4))
    extra = (torch.eye(4).repeat(4, 1, 1),) if which == "mv" else ()
    guid(render, pu, *cam, *extra, rgb_as_latents=True)
    assert order == ["noise", "t"] and jobs[0]["latent_mode"] is True and jobs[0]["post_noise"] is None
    assert tuple(jobs[0]["noise"].shape) == (4, 4, guid.image_size // 8, guid.image_size // 8)
    # image mode on the same guidance still draws the posterior sample first
    guid.posterior_noise_fn = lambda like: (order.append("posterior"), torch.zeros_like(like))[1]
    del order[:]
    guid(torch.zeros(4, 8, 8, 3).as_subclass(_OnDevice), pu, *cam, *extra)
    assert order == ["posterior", "noise", "t"] and not jobs[1]["latent_mode"] and jobs[1]["post_noise"] is not None
