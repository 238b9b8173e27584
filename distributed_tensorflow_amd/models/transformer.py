"""BERT-base (post-LN encoder, MLM + NSP heads) and GPT-2 (pre-LN causal decoder, tied LM head).

BASELINE.json configs: "BERT-base seq=512 MultiWorkerMirroredStrategy" and "GPT-2-medium fp8 weights
MirroredStrategy". Dense layers run on the MFMA GEMM with fused bias/GELU epilogues; LayerNorm,
softmax, embeddings and the vocab cross-entropy on their HIP kernels. ``fp8=True`` runs the
projection GEMMs of the transformer blocks with OCP e4m3 operands (CDNA4 fp8 MFMA, per-tensor
delayed scaling — ops.fp8).
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ..ops import decode as decode_ops
from ..ops import mha as attn_ops
from ..keras import layers as KL
from ..keras.models import Model
from ..ops.conv import ResidualGradLink

# post-LN blocks (BERT): the residual gradient of a sublayer's input is added by the sublayer's first projection's
# data-gradient GEMM in its store pass, in place in the parked buffer (no clone, no add kernel): BERT-base 19.60 ->
# 19.40 ms/step, bitwise-equal losses
RES_LINK = True
# pre-LN blocks (GPT-2): the residual gradient is added in the LayerNorm backward's store pass (GPT-2-medium bf16
# 35.50 -> 35.35, fp8 34.84 -> 34.48 ms/step, bitwise-equal results)
LN_LINK = True


class _Proj(KL.Layer):
    """Dense [units, in] with optional fp8 forward."""

    def __init__(self, units, activation=None, fp8=False, init_std=0.02, single_consumer=False, **kw):
        super().__init__(**kw)
        self.units, self.activation, self.fp8, self.init_std = units, activation, fp8, init_std
        # the output feeds exactly one _Proj (FFN1 -> FFN2): its activation backward may be fused downstream
        self.single_consumer = single_consumer

    def build(self, input_shape):
        from ..keras.initializers import TruncatedNormal
        self.kernel = self.add_weight("kernel", (self.units, input_shape[-1]), TruncatedNormal(0.0, self.init_std))
        self.bias = self.add_weight("bias", (self.units,), "zeros")
        self.built = True

    def call(self, x, training=None, link=None, cache=None):
        if cache is not None:
            # inference with a KV cache runs from the bf16 shadow, also for an fp8 model (sampling during training must
            # not touch the fp8 scaling state); the one-token decode step is a weight stream (ops.dense_skinny)
            if x.shape[-2] == 1:
                return decode_ops.step_dense(x, self.kernel, self.bias, self.activation)
            return ops.dense(x, self.kernel, self.bias, act=self.activation)
        if self.fp8 and x.is_cuda:
            from ..ops.fp8 import dense_fp8
            return dense_fp8(x, self.kernel, self.bias, self.activation, self, getattr(self, "_fp8_next", None))
        return ops.dense(x, self.kernel, self.bias, act=self.activation, link=link, tag_act=self.single_consumer)


class MultiHeadSelfAttention(KL.Layer):
    def __init__(self, hidden, heads, dropout=0.1, causal=False, fp8=False, **kw):
        super().__init__(**kw)
        self.heads, self.dropout, self.causal = heads, dropout, causal
        self.qkv = _Proj(3 * hidden, fp8=fp8)
        self.out = _Proj(hidden, fp8=fp8)

    def call(self, x, mask=None, training=None, link=None, cache=None, layer=None, append=False):
        if cache is not None:
            return self._call_cached(x, cache, layer, append)
        o = attn_ops.attention_packed(self.qkv(x, link=link), self.heads, causal=self.causal, mask=mask,
                                      dropout=self.dropout, training=training)
        return self.out(o)

    def _call_cached(self, x, cache, layer, append=False):
        """Inference with a KV cache (ops.decode.KVCache): S > 1 is the prefill of an empty cache (the causal
        attention kernel, plus a copy of K and V into the cache), S == 1 a decode step (append, then attend);
        append=True with S > 1 appends the chunk to a filled cache (store at lens + s, then attend_chunk)."""
        qkv = self.qkv(x, cache=cache)
        if x.shape[1] == 1:
            cache.store(layer, qkv)
            o = cache.attend(layer, qkv)
        elif append:
            cache.store(layer, qkv)
            o = cache.attend_chunk(layer, qkv)
        else:
            o = attn_ops.attention_packed(qkv, self.heads, causal=True, dropout=0.0, training=False)
            cache.store(layer, qkv)
        return self.out(o, cache=cache)


class BertLayer(KL.Layer):
    def __init__(self, hidden=768, heads=12, ffn=3072, dropout=0.1, **kw):
        super().__init__(**kw)
        self.att = MultiHeadSelfAttention(hidden, heads, dropout)
        self.ln1 = KL.LayerNormalization(epsilon=1e-12)
        self.ff1 = _Proj(ffn, activation="gelu", single_consumer=True)
        self.ff2 = _Proj(hidden)
        self.ln2 = KL.LayerNormalization(epsilon=1e-12)
        self.dropout = dropout

    def call(self, x, mask=None, training=None):
        # residual gradients of x join the data-gradient GEMM of the branch's first projection (ResidualGradLink)
        l1, l2 = (ResidualGradLink(), ResidualGradLink()) if (RES_LINK and training and x.is_cuda
                                                              and torch.is_grad_enabled()) else (None, None)
        a = self.att(x, mask, training=training, link=l1)
        # (into_ln: each residual sum is formed inside the LayerNorm pass that reads it first)
        x = self.ln1(ops.add_dropout(x, a, self.dropout, bool(training), link=l1, into_ln=True))
        f = self.ff2(self.ff1(x, link=l2))
        return self.ln2(ops.add_dropout(x, f, self.dropout, bool(training), link=l2, into_ln=True))


class BertModel(Model):
    """BERT encoder with MLM (tied decoder) and NSP heads. Inputs: ids, type_ids, attention mask."""

    def __init__(self, vocab=30522, hidden=768, layers=12, heads=12, ffn=3072, max_pos=512, type_vocab=2,
                 dropout=0.1, name="bert", **kw):
        super().__init__(name=name, **kw)
        self.cfg = dict(vocab=vocab, hidden=hidden, layers=layers, heads=heads, ffn=ffn, max_pos=max_pos)
        from ..keras.initializers import TruncatedNormal
        # vocab padded to a multiple of 64 (MFMA tiles); padded logits carry a -1e9 bias -> zero probability
        self.vocab, self.vocab_p = vocab, (vocab + 63) // 64 * 64
        self.word = self.add_weight("embeddings/word", (self.vocab_p, hidden), TruncatedNormal(0.0, 0.02))
        self.pos = self.add_weight("embeddings/position", (max_pos, hidden), TruncatedNormal(0.0, 0.02))
        self.typ = self.add_weight("embeddings/type", (type_vocab, hidden), TruncatedNormal(0.0, 0.02))
        self.emb_ln = KL.LayerNormalization(epsilon=1e-12)
        self.blocks = [BertLayer(hidden, heads, ffn, dropout) for _ in range(layers)]
        self.mlm_dense = _Proj(hidden, activation="gelu")
        self.mlm_ln = KL.LayerNormalization(epsilon=1e-12)
        self.mlm_bias = self.add_weight("mlm/bias", (self.vocab_p,), "zeros")
        with torch.no_grad():
            self.mlm_bias[vocab:] = -1e9
        self.pool = _Proj(hidden)
        self.nsp = _Proj(2)
        self.dropout = dropout
        self.built = True

    def encode(self, ids, type_ids=None, attn_mask=None, training=None):
        x = ops.embedding(ids, self.word, self.pos, type_ids, self.typ)
        x = ops.dropout(self.emb_ln(x), self.dropout, training=bool(training))
        mask = None
        if attn_mask is not None:
            mask = (1.0 - attn_mask.float()) * -10000.0
        for b in self.blocks:
            x = b(x, mask, training=training)
        return x

    def mlm_logits(self, h):
        t = self.mlm_ln(self.mlm_dense(h))
        return ops.dense(t, self.word, self.mlm_bias)

    def call(self, inputs, training=None):
        if isinstance(inputs, dict):
            ids, tids, am = inputs["input_ids"], inputs.get("token_type_ids"), inputs.get("attention_mask")
            mpos = inputs.get("masked_positions")
        else:
            ids, tids, am, mpos = inputs, None, None, None
        h = self.encode(ids, tids, am, training=training)
        if mpos is not None:  # gather the masked positions only (BERT pretraining)
            B, S, Hd = h.shape
            idx = (mpos + torch.arange(B, device=mpos.device)[:, None] * S).reshape(-1)
            h = ops.gather_rows(h.reshape(B * S, Hd), idx).reshape(B, -1, Hd)
        return self.mlm_logits(h)

    def nsp_logits(self, h):
        return self.nsp(torch.tanh(self.pool(h[:, 0]).float()).to(h.dtype))


class GPT2Block(KL.Layer):
    def __init__(self, hidden, heads, dropout=0.1, fp8=False, **kw):
        super().__init__(**kw)
        self.ln1 = KL.LayerNormalization(epsilon=1e-5)
        self.att = MultiHeadSelfAttention(hidden, heads, dropout, causal=True, fp8=fp8)
        self.ln2 = KL.LayerNormalization(epsilon=1e-5)
        self.fc = _Proj(4 * hidden, activation="gelu", fp8=fp8, single_consumer=True)
        self.proj = _Proj(hidden, fp8=fp8)
        if fp8:  # FFN1's output feeds only FFN2: fp8 operands from FFN1's epilogue (ops.fp8 _FUSE); untracked
            object.__setattr__(self.fc, "_fp8_next", self.proj)
        self.dropout = dropout
        object.__setattr__(self, "out_into_ln", False)  # set by GPT2: the output's first reader is a LayerNorm

    def call(self, x, training=None, cache=None, layer=None, append=False):
        if cache is not None:  # inference with a KV cache: no dropout, no gradient links
            x = ops.add(x, self.att(self.ln1(x), training=False, cache=cache, layer=layer, append=append))
            return ops.add(x, self.proj(self.fc(self.ln2(x), cache=cache), cache=cache))
        # the residual gradient of each half-block's input joins its LayerNorm's backward (ResidualGradLink)
        l1, l2 = (ResidualGradLink(), ResidualGradLink()) if (LN_LINK and training and x.is_cuda
                                                              and torch.is_grad_enabled()) else (None, None)
        # (into_ln: the residual sum is formed inside the LayerNorm pass that reads it first — ln2 here; the block
        # output only when the owning GPT2 feeds it to the next block's ln1 or ln_f, out_into_ln)
        x = ops.add_dropout(x, self.att(self.ln1(x, link=l1), training=training), self.dropout, bool(training),
                            link=l1, into_ln=True)
        return ops.add_dropout(x, self.proj(self.fc(self.ln2(x, link=l2))), self.dropout, bool(training), link=l2,
                               into_ln=self.out_into_ln)


class GPT2(Model):
    def __init__(self, vocab=50257, ctx=1024, hidden=1024, layers=24, heads=16, dropout=0.1, fp8=False,
                 name="gpt2", **kw):
        super().__init__(name=name, **kw)
        # per-bucket optimizer update during backward (parallel.strategy): round 4, with the plain GEMMs on hipBLASLt,
        # it pays for bf16 (256.0k / 255.6k vs 251.2k / 251.3k tok/s) and no longer for fp8 (248.6k / 258.2k vs
        # 256.9k / 256.5k, with 3-6 ms more host issue time); round 3 had measured the opposite (fp8 +2%, bf16 -1%)
        self.overlap_update = not fp8
        self.cfg = dict(vocab=vocab, ctx=ctx, hidden=hidden, layers=layers, heads=heads, fp8=fp8)
        from ..keras.initializers import TruncatedNormal
        # vocab padded to a multiple of 64 for the MFMA tiles (padded logits are masked out of the loss)
        self.vocab = vocab
        self.vocab_p = (vocab + 63) // 64 * 64
        self.wte = self.add_weight("wte", (self.vocab_p, hidden), TruncatedNormal(0.0, 0.02))
        self.wpe = self.add_weight("wpe", (ctx, hidden), TruncatedNormal(0.0, 0.01))
        self.blocks = [GPT2Block(hidden, heads, dropout, fp8) for _ in range(layers)]
        for b in self.blocks:  # each block output is read first by the next block's ln1 or by ln_f
            object.__setattr__(b, "out_into_ln", True)
        self.ln_f = KL.LayerNormalization(epsilon=1e-5)
        pad = torch.zeros(self.vocab_p)
        pad[vocab:] = -1e9  # padded vocab entries never receive probability mass
        self.pad_bias = self.add_weight("lm_pad_bias", (self.vocab_p,), "zeros", trainable=False)
        with torch.no_grad():
            self.pad_bias.copy_(pad.to(self.pad_bias.device))
        self.dropout = dropout
        self.built = True

    def call(self, ids, training=None, cache=None, append=False):
        if cache is not None:
            return self._lm_head(self._hidden_cached(ids, cache, append), decode=ids.shape[1] == 1)
        x = ops.dropout(ops.embedding(ids, self.wte, self.wpe), self.dropout, training=bool(training))
        for b in self.blocks:
            x = b(x, training=training)
        return ops.dense(self.ln_f(x), self.wte, self.pad_bias)  # tied LM head, logits over vocab_p

    # ---- inference with a KV cache (ops.decode)
    def _hidden_cached(self, ids, cache, append=False):
        """Final hidden states [B, S, hidden] of an inference forward that fills `cache`: S > 1 prefills an empty
        cache, S == 1 is a decode step at positions cache.lens, and append=True with S > 1 on a cache that is not empty
        appends the chunk at positions cache.lens + s (the caller advances lens afterwards in every case).
        With append=True the positions are clamped on the device to the position table, for S == 1 too: the pad token
        of a ragged row that is already full sits at position ctx (its output is never picked, its K/V are dropped or
        rewritten). The default one-token step embeds at cache.lens as it is."""
        S = ids.shape[1]
        chunk = False
        top = self.cfg["ctx"] - 1
        if S == 1:
            x = ops.embedding(ids, self.wte, self.wpe, position_ids=cache.lens.clamp(0, top) if append else cache.lens)
        elif cache.empty:
            x = ops.embedding(ids, self.wte, self.wpe)
        elif not append:
            raise NotImplementedError("chunked prefill into a non-empty KV cache needs append=True (or GPT2.extend)")
        else:
            self._refuse_gpu_chunk(ids, cache, S, False)   # before anything is stored
            chunk = True
            # pad positions of ragged rows may run past the position table: clamped on the device, never read back
            pos = cache.lens[:, None] + torch.arange(S, device=ids.device)[None, :]
            x = ops.embedding(ids, self.wte, self.wpe, position_ids=pos.clamp_(0, top))
        for i, b in enumerate(self.blocks):
            x = b(x, training=False, cache=cache, layer=i, append=chunk)
        return self.ln_f(x)

    @staticmethod
    def _refuse_gpu_chunk(ids, cache, n, more):
        """The one GPU refusal of the append route (KVCache.attend_chunk runs S > 1 on the GPU only for a cache built
        with chunked=True; remove with that opt-in): a piece of n > 1 tokens that would land behind a filled default
        cache, now or (more: further pieces follow) once the first piece has filled it. Raised before the cache is
        touched."""
        if ids.is_cuda and n > 1 and (more or not cache.empty) and not getattr(cache, "chunked", False):
            raise NotImplementedError(f"appending {n} > 1 tokens at once to a filled KV cache needs a cache built with "
                                      "chunked=True (new_cache(..., chunked=True)); feed this one a token at a time "
                                      "(extend(chunk=1), generate(prefill_chunk=1))")

    @staticmethod
    def _fits(ids, cache):
        """ids [B, S] and the cache agree in batch and device ('cuda' names the current device)."""
        def key(d):
            d = torch.device(d)
            return d.type, (torch.cuda.current_device() if d.index is None else d.index) if d.type == "cuda" else 0
        return ids.shape[0] == cache.batch and key(ids.device) == key(cache.device)

    def extend(self, ids, cache, new_lens=None, chunk=None):
        """Feed ids [B, S] (right-padded, new_lens [B] valid tokens per row, default S) into `cache` behind what it
        holds, in pieces of at most `chunk` tokens (default: all at once) -> logits [B, vocab_p] after each row's last
        valid token. cache.lens advances per row by the valid count only; no device value is read on the host.
        A row with new_lens[b] == 0 takes nothing, and its returned logits are undefined (those of a pad token).

        Room is the caller's to guarantee (checking it would be a host read of lens; `generate` does it once per
        call): every row needs lens[b] + new_lens[b] <= min(cache.capacity, ctx). Past the capacity `store` drops
        K/V silently and past ctx positions are clamped to the last table row, so an overfull row returns logits that
        mean nothing, without an error.

        Invariant (the one the ragged prefill of `generate` relies on): a position at or past lens is always rewritten
        before anything attends to it. A piece stores K/V of its pad tokens past a short row's valid end, but lens
        stops at that end, so the next piece or decode step of the row overwrites them first.

        On the GPU the first piece into an empty cache runs the prefill kernel. Behind a filled cache a piece of more
        than one token runs the multi-token append kernel (ops.decode.KVCache.attend_chunk) when the cache was built
        with chunked=True (new_cache(..., chunked=True)); on a default cache pieces are single tokens (chunk=1: the
        decode step's kernels) and anything else raises NotImplementedError before the cache is touched, with no eager
        fallback."""
        ids = ids.long()
        B, S = ids.shape
        dev = ids.device
        if not self._fits(ids, cache):
            raise ValueError(f"extend: ids {tuple(ids.shape)} on {dev} against a cache of batch {cache.batch} on "
                             f"{cache.device}")
        if S < 1:
            raise ValueError("extend needs at least one token")
        step = S if chunk is None else int(chunk)
        if step < 1:
            raise ValueError(f"extend: chunk {chunk}")
        self._refuse_gpu_chunk(ids, cache, min(step, S), S > step)
        with torch.no_grad():
            if new_lens is None:
                nl = torch.full((B,), S, dtype=torch.int64, device=dev)
            else:
                nl = torch.as_tensor(new_lens).to(dev).long()
            base = torch.arange(B, device=dev)
            last = None
            for lo in range(0, S, step):
                n = min(step, S - lo)
                piece = ids[:, lo:lo + n].contiguous()
                h = self._hidden_cached(piece, cache, append=True)
                valid = (nl - lo).clamp(0, n)                  # valid tokens of each row in this piece
                rows = (valid - 1).clamp(min=0) + base * n     # (a row with none keeps its earlier pick)
                got = ops.gather_rows(h.reshape(B * n, -1), rows)
                last = got if last is None else torch.where((valid > 0)[:, None], got, last)
                cache.advance(valid)
            return self._lm_head(last.reshape(B, 1, -1), decode=True)[:, 0]

    def _lm_head(self, h, decode=False):
        if decode:
            return decode_ops.step_dense(h, self.wte, self.pad_bias)
        return ops.dense(h, self.wte, self.pad_bias)

    def new_cache(self, batch, capacity, device, chunked=False):
        """A KV cache for this model. chunked=True: on the GPU multi-token pieces behind a filled cache run the append
        kernel (extend(chunk=N), generate(cache=, prefill_chunk=N)); a default cache refuses them."""
        c = self.cfg
        return decode_ops.KVCache(c["layers"], batch, c["heads"], capacity, device, head_dim=c["hidden"] // c["heads"],
                                  chunked=chunked)

    def _pick(self, logits, temperature, top_k, gen):
        """Next token per row from logits [B, vocab_p]: argmax, or temperature / top-k sampling, over the real
        vocabulary (padded entries carry pad_bias = -1e9 and are cut off besides)."""
        lg = logits.float()[:, :self.vocab]
        if not temperature:
            return lg.argmax(-1)
        lg = lg / float(temperature)
        if top_k is not None:
            kth = lg.topk(min(int(top_k), self.vocab), -1).values[:, -1:]
            lg = lg.masked_fill(lg < kth, float("-inf"))
        return torch.multinomial(torch.softmax(lg, -1), 1, generator=gen)[:, 0]

    def generate(self, ids, max_new_tokens, *, prompt_lens=None, temperature=0.0, top_k=None, seed=None,
                 eos_token_id=None, pad_token_id=None, graph=True, cache=None, prefill_chunk=None, top_p=None,
                 repetition_penalty=None, sampler=None):
        """Continue `ids` [B, S0] by max_new_tokens tokens with a KV cache -> int64 [B, S0 + max_new_tokens].

        cache: a KVCache to continue (``last_generation["cache"]`` of an earlier call, or one filled through
        `extend`): ids / prompt_lens are then the new tokens only and follow what the cache holds; cached + new +
        generated tokens must fit min(cache.capacity, ctx) (checked with one host read of cache.lens before the token
        loop). prefill_chunk=N feeds the prompt through `extend` in pieces of N tokens (on the GPU a cache passed in
        takes pieces of more than one token only if it was built with chunked=True: see `extend`; the cache this call
        creates itself for prefill_chunk is). With both left at None the call runs as described below.

        One prefill forward over the prompt, then one single-token step per new token (decode attention over the
        cache, weight-streaming projections); on a GPU with graph=True the step is captured into a hipGraph and
        replayed. prompt_lens [B]: lengths of right-padded prompts; a row's new tokens follow its prompt directly and
        its tail is pad_token_id. temperature 0 is greedy; otherwise temperature / top-k sampling from a
        torch.Generator seeded with `seed`. After eos_token_id a row emits pad_token_id (decided on the device: the
        loop reads no device value and always runs max_new_tokens steps). The cache and the logits after the last
        token are kept in ``last_generation`` (to inspect or continue).

        sampler="fused" picks every token with ``ops.sample_logits`` (one kernel launch: penalty, temperature, top-k,
        top-p, a counter-hash draw keyed by seed, row and position, and the eos / pad / output bookkeeping). It is also
        the route whenever top_p (nucleus) or repetition_penalty is given; sampler="torch" with either raises. The
        output tokens, each row's position and its done flag live on the device, and with graph=True the sampler launch
        and the model step are one captured step: a new token is one replay with no eager device op in between. The
        same arguments give the same tokens on the CPU reference path of the sampler as on the GPU kernel for equal
        logits, eagerly and replayed, and for a row alone or among others at the same row index. The penalty applies
        to the tokens this call was given and produced (with cache=, not to what the cache already held). With all
        three left at None the torch.Generator route above runs unchanged."""
        if sampler not in (None, "torch", "fused"):
            raise ValueError(f"generate: sampler {sampler!r} (None, 'torch' or 'fused')")
        if sampler == "torch" and (top_p is not None or repetition_penalty is not None):
            raise ValueError("generate: top_p and repetition_penalty need the fused sampler")
        fused = sampler == "fused" or (sampler is None and (top_p is not None or repetition_penalty is not None))
        ids = ids.long()
        B, S0 = ids.shape
        dev = ids.device
        n_new = int(max_new_tokens)
        ctx = self.cfg["ctx"]
        if S0 + n_new > ctx:
            raise ValueError(f"prompt ({S0}) + max_new_tokens ({n_new}) exceeds the context length {ctx}")
        if S0 < 1 or n_new < 0:
            raise ValueError("generate needs a non-empty prompt and max_new_tokens >= 0")
        if cache is not None:
            if not self._fits(ids, cache):
                raise ValueError(f"generate: ids {tuple(ids.shape)} on {dev} against a cache of batch {cache.batch} on "
                                 f"{cache.device}")
            # the one host read of a call with a cache: before the token loop, outside any capture
            held, room = int(cache.lens.max()), min(cache.capacity, ctx)
            if held + S0 + n_new > room:
                raise ValueError(f"cached tokens ({held}) + new tokens ({S0}) + max_new_tokens ({n_new}) exceed "
                                 f"min(cache capacity {cache.capacity}, context length {ctx})")
        if n_new == 0 and cache is None:
            return ids.clone()
        pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
        gen = None
        if temperature and not fused:
            gen = torch.Generator(device=dev)
            gen.manual_seed(0 if seed is None else int(seed))
        with torch.no_grad():
            if prompt_lens is None:
                plens = torch.full((B,), S0, dtype=torch.int64, device=dev)
            else:
                plens = torch.as_tensor(prompt_lens).to(dev).long()
            if cache is None and prefill_chunk is None:
                cache = self.new_cache(B, S0 + n_new, dev)
                h = self._hidden_cached(ids, cache)  # prefill: K/V of all S0 positions; a pad position is rewritten
                cache.set_lens(plens)                # by the decode step that reaches it before anything attends to it
                rows = plens - 1 + torch.arange(B, device=dev) * S0
                last = ops.gather_rows(h.reshape(B * S0, -1), rows)  # each row's own last prompt position
                logits = self._lm_head(last.reshape(B, 1, -1), decode=True)[:, 0]
            else:
                if cache is None:  # (prefill_chunk given: the pieces after the first land behind a filled cache)
                    cache = self.new_cache(B, S0 + n_new, dev, chunked=True)
                logits = self.extend(ids, cache, plens, prefill_chunk)  # behind what the cache holds, in pieces

            def step(tok):
                lg = self._lm_head(self._hidden_cached(tok, cache), decode=True)
                cache.advance(1)
                return lg

            col = torch.arange(S0, device=dev)[None, :]
            out = torch.full((B, S0 + n_new), int(pad), dtype=torch.int64, device=dev)
            out[:, :S0] = torch.where(col < plens[:, None], ids, out[:, :S0])
            done = torch.zeros(B, dtype=torch.bool, device=dev)
            if fused:
                # the step reads `logits` and rewrites it in place, so a replay takes no argument and copies nothing in
                logits = logits.contiguous().clone()
                pos = plens.clone()

                def fused_step(_):
                    tok = ops.sample_logits(logits, n=self.vocab, temperature=temperature, top_k=top_k, top_p=top_p,
                                            repetition_penalty=repetition_penalty, seed=seed, out=out, pos=pos,
                                            done=done, eos=eos_token_id, pad=int(pad))
                    logits.copy_(step(tok[:, None])[:, 0])
                    return logits

            captured = None
            if graph and dev.type == "cuda":
                from ..graphs import CapturedStep
                # one stream only: a graph without parallel branches
                captured = CapturedStep(fused_step if fused else step, split=False)
            if fused:
                for t in range(n_new):
                    (captured or fused_step)(())
            else:
                for t in range(n_new):
                    tok = self._pick(logits, temperature, top_k, gen)
                    if eos_token_id is not None:
                        tok = torch.where(done, torch.full_like(tok, int(pad)), tok)
                        done = done | (tok == int(eos_token_id))
                    out.scatter_(1, (plens + t)[:, None], tok[:, None])
                    logits = (captured or step)(tok[:, None].contiguous())[:, 0]
            logits = logits.clone()
        object.__setattr__(self, "last_generation", {"cache": cache, "logits": logits, "step": captured})
        return out


def bert_base(**kw):
    return BertModel(**kw)


def gpt2_medium(fp8=False, **kw):
    return GPT2(hidden=1024, layers=24, heads=16, fp8=fp8, **kw)


def gpt2_small(fp8=False, **kw):
    return GPT2(hidden=768, layers=12, heads=12, fp8=fp8, **kw)


def count_flops_per_token(cfg, seq):
    """Approximate training FLOPs/token (6N + attention) for throughput reporting."""
    h, L = cfg["hidden"], cfg["layers"]
    n = 12 * L * h * h
    return 6 * n + 12 * L * h * seq


del math
