"""`stable-diffusion-multi-prompt-processor` (custom/amortized/models/prompt_processors/base.py:31-407 +
stable_diffusion_multi_prompt_processor.py): prompt library -> text embeddings, the first stage of the amortized workflow.

The library `<prompt_library_dir>/<prompt_library>.<format>` is read, all its splits are concatenated and the rank keeps `[rank::world]`
(base.py:171-188); every prompt is encoded as itself plus four view-dependent strings, together with the negative prompt.  The cache is
the reference's: `<cache_dir>/<md5(f"{model}-{prompt}-{type}")>.pt` with type "global" (the pooled output, one CPU fp32 [C] tensor) and
"local" (last_hidden_state, [77, C]) (utils.py:5-7, stable_diffusion_multi_prompt_processor.py:72-89), so embeddings computed by a
ScaleDreamer installation are picked up unchanged, and the other way round.  What the cache lacks is tokenized by
`tokenize_fn(list of str) -> input_ids` (default: the local CLIPTokenizer of `<model>/tokenizer`) and encoded in batches by
diffusion/text_hip.HipClipTextEncoder, which is released afterwards; the reference encodes one string per call in fp32 (base.py:298-305).
`__call__(prompt)` returns the MultiPromptUtils of multiprompt.py with the field mapping of base.py:391-406."""
from __future__ import annotations

import hashlib
import json
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from ._lib import AsdError
from .base import BaseObject, get_rank
from .registry import debug, info, register

DIRECTIONS = ("side", "front", "back", "overhead")      # order of text_embeddings_vd (base.py:100-165)
ENCODE_BATCH = 1024                                      # strings tokenized, encoded and written per round


def hash_prompt(model: str, prompt: str, type: str) -> str:
    """utils.py:5-7"""
    return hashlib.md5(f"{model}-{prompt}-{type}".encode()).hexdigest()


def direction_prompts(prompt: str, view_dependent_prompt_front: bool) -> List[str]:
    """the four strings of a prompt in DIRECTIONS order, in either form (base.py:100-165)"""
    if view_dependent_prompt_front:
        return [f"{'backside' if d == 'back' else d} view of {prompt}" for d in DIRECTIONS]
    return [f"{prompt}, {d} view" for d in DIRECTIONS]


def shard(prompt_library: Dict[str, Sequence[str]], rank: int, world: int) -> List[str]:
    """all splits, each cut to [rank::world], concatenated in the file's order (base.py:175-180)"""
    out: List[str] = []
    for split in prompt_library:
        out += list(prompt_library[split])[rank::world]
    return out


def local_tokenizer(model: str) -> Callable:
    """tokenize(list of str) -> input_ids [n, model_max_length] with the CLIPTokenizer of <model>/tokenizer: padding to max_length, then the
    reference's slice instead of truncation=True (stable_diffusion_multi_prompt_processor.py:59-66).  Nothing is downloaded."""
    state: Dict[str, object] = {}

    def tokenize(prompts):
        if "tok" not in state:
            try:
                from transformers import CLIPTokenizer
            except ImportError as e:
                raise AsdError(f"the default tokenizer needs the `transformers` package (CLIPTokenizer of {os.path.join(model, 'tokenizer')}), which is "
                               f"missing: {e}; install it or pass tokenize_fn") from e
            state["tok"] = CLIPTokenizer.from_pretrained(os.path.join(model, "tokenizer"), local_files_only=True)
        tok = state["tok"]
        n = tok.model_max_length
        rows = tok(list(prompts), padding="max_length", max_length=n).input_ids
        return torch.tensor([r[:n] for r in rows], dtype=torch.long)

    return tokenize


def has_local_text_encoder(model: str) -> bool:
    """<model>/text_encoder (config.json and weights) and <model>/tokenizer exist on this machine"""
    d = os.path.join(model, "text_encoder")
    return (os.path.isfile(os.path.join(d, "config.json")) and any(os.path.isfile(os.path.join(d, n)) for n in ("model.safetensors", "pytorch_model.bin"))
            and os.path.isdir(os.path.join(model, "tokenizer")))


def encode_in_batches(prompts: Sequence[str], tokenize_fn: Callable, encoder_factory: Callable, write: Callable, batch: int = ENCODE_BATCH) -> int:
    """tokenize and encode `prompts` `batch` strings at a time; write(prompt, pooled fp32 [C] CPU, hidden fp32 [L, C] CPU) per string.  The
    encoder is built once, when there is something to encode, and released at the end.  Returns the number of encoder calls."""
    if not prompts:
        return 0
    encoder, calls = encoder_factory(), 0
    try:
        for i in range(0, len(prompts), batch):
            part = list(prompts[i:i + batch])
            hidden, pooled = encoder(torch.as_tensor(tokenize_fn(part)))
            calls += 1
            hidden, pooled = hidden.detach().float().cpu(), pooled.detach().float().cpu()
            assert hidden.shape[0] == pooled.shape[0] == len(part)
            for j, p in enumerate(part):
                write(p, pooled[j].clone(), hidden[j].clone())        # clones: a saved view would carry the whole batch's storage
    finally:
        if hasattr(encoder, "release"):
            encoder.release()
        del encoder
    return calls


@register("stable-diffusion-multi-prompt-processor")
class StableDiffusionMultiPromptProcessor(BaseObject):
    @dataclass
    class Config(BaseObject.Config):
        prompt_library: str = "magic3d_prompt_library"
        prompt_library_dir: str = "load"
        prompt_library_format: str = "json"
        eval_prompt: Optional[str] = None
        eval_prompt_target: Optional[str] = None
        pretrained_model_name_or_path: str = "runwayml/stable-diffusion-v1-5"
        negative_prompt: str = ""
        overhead_threshold: float = 60.0
        front_threshold: float = 45.0
        back_threshold: float = 45.0
        view_dependent_prompt_front: bool = False
        use_cache: bool = True
        spawn: bool = False
        cache_dir: str = ".threestudio_cache/text_embeddings"
        use_perp_neg: bool = False
        perp_neg_f_sb: Tuple[float, float, float] = (1, 0.5, -0.606)
        perp_neg_f_fsb: Tuple[float, float, float] = (1, 0.5, +0.967)
        perp_neg_f_fs: Tuple[float, float, float] = (4, 0.5, -2.426)
        perp_neg_f_sf: Tuple[float, float, float] = (4, 0.5, -2.426)
        use_prompt_debiasing: bool = False
        use_local_text_embeddings: bool = False

    cfg: Config

    def configure(self, tokenize_fn: Optional[Callable] = None, encoder_factory: Optional[Callable] = None, rank: Optional[int] = None,
                  n_ranks: Optional[int] = None) -> None:
        """tokenize_fn(list of str) -> input_ids [n, L]; encoder_factory() -> an object called as encoder(input_ids) -> (last_hidden_state
        [n, L, C], pooled [n, C]) (and released with .release() when it has one).  Both default to the local tokenizer and the HIP encoder
        of cfg.pretrained_model_name_or_path."""
        c = self.cfg
        self._cache_dir = c.cache_dir
        self.tokenize_fn, self.encoder_factory = tokenize_fn, encoder_factory
        self.encode_calls = 0
        if c.eval_prompt is None:
            rank = get_rank() if rank is None else rank
            n_ranks = int(os.environ.get("WORLD_SIZE", max(1, torch.cuda.device_count()))) if n_ranks is None else n_ranks
            path = os.path.join(c.prompt_library_dir, c.prompt_library) + "." + c.prompt_library_format
            with open(path, "r") as f:
                self.prompt_library = shard(json.load(f), rank, n_ranks)       # each process holds its part of the library only
        else:
            self.prompt_library = [c.eval_prompt] + ([c.eval_prompt_target] if c.eval_prompt_target is not None else [])
        self._in_library = set(self.prompt_library)
        self.negative_prompt = c.negative_prompt
        info(f"Using prompt library located in [{c.prompt_library}] and negative prompt [{self.negative_prompt}]")
        if c.use_prompt_debiasing:
            raise NotImplementedError("Prompt debiasing is not implemented yet")
        self.prompts_vd = {p: direction_prompts(p, c.view_dependent_prompt_front) for p in self.prompt_library}
        self.negative_prompts_vd = [self.negative_prompt for _ in DIRECTIONS]      # the directions leave a negative prompt as it is
        self.prepare_text_embeddings()
        self.load_text_embeddings()

    def cache_path(self, prompt: str, type: str) -> str:
        return os.path.join(self._cache_dir, f"{hash_prompt(self.cfg.pretrained_model_name_or_path, prompt, type)}.pt")

    def all_strings(self) -> List[str]:
        """every distinct string that needs an embedding, in the reference's order (base.py:232-241)"""
        vds = [s for p in self.prompts_vd for s in self.prompts_vd[p]]
        return list(dict.fromkeys(self.prompt_library + [self.negative_prompt] + vds + self.negative_prompts_vd))

    def prepare_text_embeddings(self) -> None:
        os.makedirs(self._cache_dir, exist_ok=True)
        todo = [s for s in self.all_strings()
                if not (self.cfg.use_cache and os.path.exists(self.cache_path(s, "global")) and os.path.exists(self.cache_path(s, "local")))]
        if not todo:
            debug("Text embeddings of every prompt are already in cache, skip processing.")
            return
        model = self.cfg.pretrained_model_name_or_path
        tokenize_fn = self.tokenize_fn or local_tokenizer(model)
        factory = self.encoder_factory
        if factory is None:
            def factory():
                from .diffusion.text_hip import HipClipTextEncoder

                return HipClipTextEncoder.from_pretrained(model, device=self.device)

        def write(prompt, pooled, hidden):
            torch.save(pooled, self.cache_path(prompt, "global"))
            torch.save(hidden, self.cache_path(prompt, "local"))

        info(f"Encoding {len(todo)} strings for model {model}.")
        self.encode_calls += encode_in_batches(todo, tokenize_fn, factory, write)

    def _load(self, prompt: str, type: str) -> torch.Tensor:
        path = self.cache_path(prompt, type)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{type.capitalize()} Text embedding file {path} for model {self.cfg.pretrained_model_name_or_path} and prompt "
                                    f"[{prompt}] not found.")
        return torch.load(path, map_location="cpu").to(self.device)

    def load_text_embeddings(self) -> None:
        """the tables, on the device: per prompt (and for the negative prompt) the global [C], the local [77, C] and the four view-dependent
        local embeddings [4, 77, C] (utils.py:43-58)"""
        self.global_text_embeddings: Dict[str, torch.Tensor] = {}
        self.local_text_embeddings: Dict[str, torch.Tensor] = {}
        self.text_embeddings_vd: Dict[str, torch.Tensor] = {}
        for p, vds in list(self.prompts_vd.items()) + [(self.negative_prompt, self.negative_prompts_vd)]:
            self.global_text_embeddings[p] = self._load(p, "global")
            self.local_text_embeddings[p] = self._load(p, "local")
            self.text_embeddings_vd[p] = torch.stack([self._load(s, "local") for s in vds], dim=0)
        debug("Loaded text embeddings.")

    def __call__(self, prompt: Union[str, List[str]]):
        from .multiprompt import MultiPromptUtils

        prompt = [prompt] if isinstance(prompt, str) else prompt
        for p in prompt:
            if p not in self._in_library:
                raise ValueError(f"Prompt [{p}] is not in the prompt library.")
        c = self.cfg
        return MultiPromptUtils(
            global_text_embeddings=[self.global_text_embeddings[p] for p in prompt],
            local_text_embeddings=[self.local_text_embeddings[p] for p in prompt],
            uncond_text_embeddings=self.local_text_embeddings[self.negative_prompt],
            text_embeddings_vd=[self.text_embeddings_vd[p] for p in prompt],
            uncond_text_embeddings_vd=self.text_embeddings_vd[self.negative_prompt],
            use_perp_neg=c.use_perp_neg, overhead_threshold=c.overhead_threshold, front_threshold=c.front_threshold, back_threshold=c.back_threshold,
            perp_neg_f_sb=tuple(c.perp_neg_f_sb), perp_neg_f_fsb=tuple(c.perp_neg_f_fsb), perp_neg_f_fs=tuple(c.perp_neg_f_fs),
            perp_neg_f_sf=tuple(c.perp_neg_f_sf), use_local_text_embeddings=c.use_local_text_embeddings)
