"""Model adapters behind build_chatbot (reference: neural_chat/models/base_model.py:64-420 and model_utils.py
load_model :578-1000 / predict_stream :1061-1380 / predict :1383-1600, reduced to the HF + weight-only-quantised path).

Generation runs on the GPU in one of two ways:
 * greedy, single beam, Llama-class model  -> the fused decode engine (runtime/engine.py: prompt pass on the MFMA
   GEMMs, then hipGraph-replayed decode steps), tokens streamed as they are produced;
 * anything else (sampling, beams, other architectures) -> `model.generate` of the HF model whose linears are
   QuantizedLinearQBits modules, with a TextIteratorStreamer on a worker thread exactly like the reference
   (model_utils.py:1249).
"""
import time
from threading import Thread

from ..config import GenerationConfig
from ..prompts import get_conv_template


class BaseModel:
    def __init__(self, model_name="", task=""):
        self.model_name = model_name
        self.task = task
        self.model = None
        self.tokenizer = None
        self.engine = None
        self.device = "cuda"
        self.conv_template = None
        self.use_cache = True

    # ---- reference BaseModel surface -------------------------------------------------------------------------
    def match(self):
        return True

    def get_default_conv_template(self):
        return get_conv_template("raw")

    def load_model(self, kwargs: dict):
        """kwargs keys as the reference builds them in chatbot.py (model_name, tokenizer_name, device,
        optimization_config, use_cache, ...)."""
        import torch
        from transformers import AutoTokenizer

        from ...transformers import AutoModelForCausalLM, MixedPrecisionConfig

        self.model_name = kwargs["model_name"]
        self.device = kwargs.get("device", "cuda")
        self.use_cache = kwargs.get("use_cache", True)
        if kwargs.get("use_neural_speed") or kwargs.get("use_vllm") or kwargs.get("gguf_model_path"):
            raise NotImplementedError("QBits: Neural Speed / GGUF / vLLM back ends are outside the MI355X path")
        if self.device != "cuda":
            raise RuntimeError("QBits: the MI355X backend has no %s path; use device='cuda'" % self.device)
        opt = kwargs.get("optimization_config")
        self.tokenizer = AutoTokenizer.from_pretrained(kwargs.get("tokenizer_name") or self.model_name)
        if opt is None or isinstance(opt, MixedPrecisionConfig):
            dt = getattr(torch, (opt.dtype if opt is not None else "float16"))
            self.model = AutoModelForCausalLM.from_pretrained(self.model_name, torch_dtype=dt, device_map="cuda")
        else:  # weight-only quantisation at load time, reference model_utils.py:796-822
            self.model = AutoModelForCausalLM.from_pretrained(self.model_name, quantization_config=opt,
                                                              device_map="cuda")
        if kwargs.get("peft_path"):
            # reference model_utils.py load_model: PeftModel.from_pretrained(model, peft_path), kept unmerged. Here the
            # adapter goes over the blobs (llm/quantization/lora.py) and the model stays on the module path, unless
            # LoadingModelConfig(peft_on_engine=True) asks for the engine to carry the adapter unmerged
            from ...transformers.llm.quantization.lora import load_peft_adapter

            load_peft_adapter(self.model, kwargs["peft_path"])
        self.model.eval()
        self.conv_template = self.get_default_conv_template()
        self._try_engine("unmerged" if kwargs.get("peft_path") and kwargs.get("peft_on_engine") else None)

    def _try_engine(self, adapters=None):
        """Build the fused decode engine when the model is a quantised Llama-class decoder; otherwise stay on the
        module path (not an error). `adapters`: optimize_transformers' keyword."""
        self.engine = None
        if not hasattr(self.model, "quantization_config"):
            return
        try:
            from ...runtime.engine import engine_supports, optimize_transformers

            if not engine_supports(self.model.config)[0]:  # the acceptance rule shared with `generate` and the TP host
                return
            ctx = int(min(getattr(self.model.config, "max_position_embeddings", 2048) or 2048, 8192))
            self.engine = optimize_transformers(self.model, max_ctx=ctx, adapters=adapters)
        except RuntimeError:
            self.engine = None

    def prepare_prompt(self, query, config=None):
        conv = self.conv_template.copy()
        if conv.roles[0] and conv.roles[0] in query and conv.roles[1] in query:
            return query  # the caller already applied a template (reference base_model.py:174-180)
        conv.append_message(conv.roles[0], query)
        conv.append_message(conv.roles[1], None)
        return conv.get_prompt()

    def predict_stream(self, query, origin_query="", config=None):
        """-> (generator of text pieces, link) like the reference (base_model.py:150-273: `return response, link`;
        `link` is the retrieval plugin's source list, always empty here — plugins are out of scope). With
        config.return_stats the reference's trailing stats block follows the text (model_utils.py:1340-1380,
        format v1 / v2)."""
        config = config or GenerationConfig()
        prompt = self.prepare_prompt(query, config)
        return self._stream(prompt, config), []

    def predict(self, query, origin_query="", config=None):
        config = config or GenerationConfig()
        prompt = self.prepare_prompt(query, config)
        stats = config.return_stats
        config.return_stats = False
        try:
            return "".join(self._stream(prompt, config))
        finally:
            config.return_stats = stats

    def score_prompt(self, prompt, n_top=0):
        """Log-probabilities the model assigns to the tokens of `prompt` itself (tokenised as `predict` tokenises a plain
        completion): one entry per prompt token in the shape of `last_logprobs` entries (`token_id`, `token`, `logprob`,
        `top` = `n_top` alternatives as (id, string, logprob), `text_offset`). The first token has nothing in front of
        it: `logprob` None, `top` empty. One scored prompt pass on the fused engine (`WoqDecoderEngine.score`)."""
        if self.engine is None:
            raise RuntimeError("QBits: scoring a prompt needs the fused engine")
        tok = self.tokenizer
        ids = [int(t) for t in tok(prompt, return_tensors="pt").input_ids[0].tolist()]
        lps, tops = self.engine.score(ids, logprobs=int(n_top)) if len(ids) > 1 else ([], [])
        entries = []
        for i, t in enumerate(ids):
            top = [] if i == 0 else [(int(j), tok.decode([int(j)]), float(v)) for j, v in tops[i - 1] if j >= 0]
            entries.append({"token_id": t, "token": tok.decode([t]), "logprob": None if i == 0 else float(lps[i - 1]),
                            "top": top,
                            "text_offset": len(tok.decode(ids[:i], skip_special_tokens=True)) if i else 0})
        return entries

    # ---- generation ----------------------------------------------------------------------------------------------
    def _stream(self, prompt, config):
        ids = self.tokenizer(prompt, return_tensors="pt").input_ids
        n_in = int(ids.shape[1])
        t_start = time.time()
        first = [None]
        n_out = [0]
        self.last_logprobs = []  # one dict per emitted token when config.logprobs is set (_note_logprobs)
        # one sequence, one beam: the fused engine — greedy chains on the device; sampling (the reference's default:
        # do_sample, temperature, top_k, top_p) and the repetition penalty pick the next token with the device sampler
        # (bad_words_ids, guided_choice and guided_regex ride the engine too: a token guide its sampler follows)
        engine_ok = config.num_beams == 1 and (config.num_return_sequences or 1) == 1 and not config.force_words_ids
        guide = self.request_guide(config)
        if guide is not None and self.engine is not None and not self.engine.native_sampler_supports(guide=guide):
            engine_ok = False
        if guide is None and config.bad_words_ids:  # words the guide's builder does not take: Hugging Face's loop
            engine_ok = False

        # rolling KV cache (config.ctx_size / n_keep / n_discard): a request longer than the engine's cache stays on
        # the engine, which drops old positions behind its attention sinks (runtime.streaming)
        streaming = self._streaming(config)

        def pieces():
            if engine_ok and self.engine is not None and (n_in + config.max_new_tokens <= self.engine.cfg.max_ctx
                                                          or streaming is not None):
                yield from self._engine_stream(ids[0].tolist(), config, n_out)
            elif getattr(config, "logprobs", None) is not None:
                raise RuntimeError("QBits: logprobs need the fused engine")
            elif getattr(config, "guided_choice", None) or getattr(config, "guided_regex", None):
                raise RuntimeError("QBits: guided_choice / guided_regex need the fused engine")
            else:
                yield from self._hf_stream(ids, config, n_out)

        for text in pieces():
            if not text:
                continue
            if first[0] is None:
                first[0] = time.time()
            yield text
        if config.return_stats:
            dur = int((time.time() - t_start) * 1000)
            ftl = int(((first[0] or time.time()) - t_start) * 1000)
            per = dur / n_out[0] if n_out[0] else 0
            if config.format_version == "v1":
                yield "END_OF_STREAM_STATS={}".format({"input_token_len": n_in, "output_token_len": n_in + n_out[0],
                                                       "duration": dur, "first_token_latency": ftl,
                                                       "msecond_per_token": per})
            else:
                stats = {"input_token_len": str(n_in), "output_token_len": str(n_in + n_out[0]),
                         "duration": "%d ms" % dur, "first_token_latency": "%d ms" % ftl,
                         "msecond_per_token": "%s ms" % per}
                yield "\n| {:<22} | {:<27} |\n".format("Key", "Value")
                yield "| " + "-" * 22 + " | " + "-" * 27 + " |" + "\n"
                for k, v in stats.items():
                    yield "| {:<22} | {:<27} |\n".format(k, v)

    def _note_logprobs(self, out, t, lp, top):
        """One entry of `last_logprobs` for token `t` about to be appended to the emitted ids `out`: its id, decoded
        string, log-probability under the raw model distribution, the `top` alternatives as (id, string, logprob) and
        `text_offset`, where the token starts in the returned text."""
        tok = self.tokenizer
        self.last_logprobs.append({
            "token_id": int(t), "token": tok.decode([int(t)]), "logprob": float(lp),
            "top": [(int(i), tok.decode([int(i)]), float(v)) for i, v in top if i >= 0],
            "text_offset": len(tok.decode(out, skip_special_tokens=True)) if out else 0})

    def _text_pieces(self, bursts, n_out):
        """Text pieces of an engine stream whose bursts are token lists or `(tokens, chosen_lps, top)`; the latter fill
        `last_logprobs`. EOS is left out of the text, the count `n_out` and the records."""
        tok = self.tokenizer
        eos = tok.eos_token_id
        out, shown = [], ""
        for burst in bursts:
            new, lps, tops = burst if isinstance(burst, tuple) else (burst, None, None)
            for j, t in enumerate(new):
                if eos is not None and t == eos:
                    continue
                if lps is not None:
                    self._note_logprobs(out, t, lps[j], tops[j])
                out.append(t)
                n_out[0] += 1
            text = tok.decode(out, skip_special_tokens=True)
            if not text.endswith("\ufffd"):  # hold back incomplete multi-byte pieces, like TextIteratorStreamer
                yield text[len(shown):]
                shown = text

    def request_guide(self, config):
        """The TokenGuide of a request, or None: `guided_choice` / `guided_regex` over this tokenizer's bytes
        (ValueError with the builder's message for a pattern it does not take, for both at once and for a model without
        an EOS token), else `bad_words_ids` as Hugging Face's NoBadWordsLogitsProcessor. Built once per tokenizer and
        pattern."""
        from ...runtime.guide import TokenGuide, token_bytes

        choice, regex = getattr(config, "guided_choice", None), getattr(config, "guided_regex", None)
        bad = getattr(config, "bad_words_ids", None)
        if choice is not None and regex is not None:
            raise ValueError("guided_choice and guided_regex cannot be used together")
        if choice is None and regex is None and not bad:
            return None
        if self.engine is None:
            return None  # (_stream says what needs the engine; bad_words_ids stay with Hugging Face's loop)
        vocab = int(self.engine.cfg.vocab)
        cache = self.__dict__.setdefault("_guide_cache", {})
        if choice is None and regex is None:
            key = ("bad_words", tuple(tuple(int(t) for t in w) for w in bad))
            if key not in cache:
                try:
                    cache[key] = TokenGuide.from_bad_words(bad, vocab)
                except ValueError:
                    cache[key] = None  # what the builder does not take keeps Hugging Face's loop
            return cache[key]
        key = ("choice", tuple(choice)) if choice is not None else ("regex", regex)
        if key not in cache:
            tok = self.tokenizer
            if tok.eos_token_id is None:
                raise ValueError("guided decoding needs a tokenizer with an EOS token (the guide ends the text with it)")
            if "bytes" not in cache:
                pieces = token_bytes(tok)
                cache["bytes"] = (pieces + [b""] * vocab)[:vocab]  # the model's head may be padded past the tokenizer
            if choice is not None and (not choice or not all(isinstance(c, str) and c for c in choice)):
                raise ValueError("guided_choice is a non-empty list of non-empty strings")
            while len(cache) > 64:  # a bound on what a server keeps
                cache.pop(next(k for k in cache if k != "bytes"))
            cache[key] = (TokenGuide.from_choices(choice, cache["bytes"], [tok.eos_token_id]) if choice is not None
                          else TokenGuide.from_regex(regex, cache["bytes"], [tok.eos_token_id]))
        return cache[key]

    @staticmethod
    def _streaming(config):
        """the request's StreamingConfig (GenerationConfig.ctx_size / n_keep / n_discard), None when none is set"""
        from ...runtime.streaming import streaming_from_keywords

        return streaming_from_keywords(getattr(config, "ctx_size", None), getattr(config, "n_keep", None),
                                       getattr(config, "n_discard", None))

    def _sampler_controls(self, config):
        """the request's sampling controls as `iter_sampled_auto` keywords (neutral values where the config has none)"""
        return dict(guide=self.request_guide(config), presence_penalty=getattr(config, "presence_penalty", 0.0) or 0.0,
                    frequency_penalty=getattr(config, "frequency_penalty", 0.0) or 0.0,
                    min_p=(getattr(config, "min_p", 0.0) or 0.0) if config.do_sample else 0.0,  # a warper: sampling only
                    logit_bias=dict(getattr(config, "logit_bias", None) or {}), seed=getattr(config, "seed", None))

    def _engine_stream(self, ids, config, n_out):
        """The request on the fused engine, handed to the text stream one token at a time. The reference's default
        request (sampling + repetition penalty), the other penalties, a bias and a guide need a sampler: tokens are chosen
        on the device, by the engine's native sampler where it covers the request, else by runtime.request.DeviceSampler
        (a penalty or a bias with temperature 0 is a greedy request over the penalised scores: the sampler's argmax).
        Everything else is the greedy chain."""
        from ...runtime.engine import iter_sampled_auto

        eos = self.tokenizer.eos_token_id
        ctl = self._sampler_controls(config)
        common = dict(burst=1, eos=() if eos is None else (eos,), logprobs=getattr(config, "logprobs", None),
                      streaming=self._streaming(config))
        if config.do_sample or (config.repetition_penalty or 1.0) != 1.0 or ctl["presence_penalty"] \
                or ctl["frequency_penalty"] or ctl["logit_bias"] or ctl["guide"] is not None:
            bursts = iter_sampled_auto(self.engine, ids, config.max_new_tokens, do_sample=config.do_sample,
                                       temperature=config.temperature, top_k=config.top_k, top_p=config.top_p,
                                       repetition_penalty=config.repetition_penalty, **common, **ctl)
        else:
            bursts = self.engine.iter_generate(ids, config.max_new_tokens, **common)
        yield from self._text_pieces(bursts, n_out)

    def _hf_stream(self, ids, config, n_out):
        import torch
        from transformers import TextIteratorStreamer

        ctl = self._sampler_controls(config)
        if ctl["presence_penalty"] or ctl["frequency_penalty"] or ctl["logit_bias"]:
            # HF's generate has no presence / frequency penalty and no OpenAI logit_bias: refuse, never ignore
            raise RuntimeError("QBits: presence_penalty, frequency_penalty and logit_bias need the fused engine (one "
                               "sequence, one beam, prompt + max_new_tokens within its context)")
        streamer = TextIteratorStreamer(self.tokenizer, skip_prompt=True, skip_special_tokens=True)
        gen = dict(max_new_tokens=config.max_new_tokens, do_sample=config.do_sample, num_beams=config.num_beams,
                   use_cache=config.use_cache, repetition_penalty=config.repetition_penalty,
                   num_return_sequences=config.num_return_sequences, pad_token_id=self.tokenizer.eos_token_id)
        if config.do_sample:
            gen.update(temperature=config.temperature, top_k=config.top_k, top_p=config.top_p)
            if ctl["min_p"]:
                gen.update(min_p=ctl["min_p"])
        err = []
        result = []
        seed = ctl["seed"]

        def work():
            try:
                if seed is not None and config.do_sample:  # HF's loop draws from torch's default generator
                    torch.manual_seed(int(seed) & (2 ** 63 - 1))
                with torch.no_grad():
                    result.append(self.model.generate(ids.to("cuda"), streamer=streamer, **gen))
            except Exception as e:  # surfaced on the consumer side, like the reference's errors_queue
                err.append(e)
                streamer.end()

        th = Thread(target=work)
        th.start()
        for text in streamer:
            yield text
        th.join()
        if err:
            raise err[0]
        if result:
            n_out[0] = int(result[0].shape[-1]) - int(ids.shape[1])


class LlamaModel(BaseModel):
    def match(self):
        return "llama" in self.model_name.lower()

    def get_default_conv_template(self):
        return get_conv_template("llama-2")


class MistralModel(BaseModel):
    def match(self):
        return "mistral" in self.model_name.lower()

    def get_default_conv_template(self):
        return get_conv_template("mistral")


class NeuralChatModel(BaseModel):
    def match(self):
        return "neural-chat" in self.model_name.lower()

    def get_default_conv_template(self):
        return get_conv_template("neural-chat-7b-v3")
