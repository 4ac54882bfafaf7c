"""OpenAI-compatible text-chat routes over a chatbot built by `build_chatbot` — the request path of SURVEY §3.4:
FastAPI `POST /v1/chat/completions` (reference neural_chat/server/restful/textchat_api.py:482) -> `chatbot.predict` /
`chatbot.predict_stream` -> the quantised model on the GPU.

Same routes, request fields, response objects and error shape as the reference's router (textchat_api.py:374-713,
wire objects openai_protocol.py:32-230); what differs is behind them:
 * one process = one GPU = one decode engine, so requests are serialised on a lock and run on a worker thread (the
   event loop keeps answering /health); the reference's DeepSpeed fan-out to worker ports (:486-528) has no
   counterpart — tensor parallelism lives inside the engine (runtime/tp.py);
 * greedy requests (temperature 0 or top_k 1 — the OpenAI defaults of this route) ride the fused engine;
 * streamed deltas are the text pieces as generated. The reference re-splits every piece on whitespace
   (:337-345) and so drops the spaces between words; that quirk is not reproduced.
"""
import json
import threading
import time
import types
import uuid
from typing import Any, Dict, List, Optional, Union

from fastapi import APIRouter
from fastapi.concurrency import run_in_threadpool
from fastapi.responses import JSONResponse, Response, StreamingResponse
from pydantic import BaseModel as _Wire

from ...config import GenerationConfig


class ChatCompletionRequest(_Wire):
    model: str
    messages: Union[str, List[Dict[str, Any]]]
    temperature: Optional[float] = 0.7
    top_p: Optional[float] = 1.0
    top_k: Optional[int] = 1
    n: Optional[int] = 1
    max_tokens: Optional[int] = None
    stop: Optional[Union[str, List[str]]] = None
    stream: Optional[bool] = False
    repetition_penalty: Optional[float] = 1.0
    presence_penalty: Optional[float] = 0.0
    frequency_penalty: Optional[float] = 0.0
    logit_bias: Optional[Dict[str, float]] = None  # token-id strings -> [-100, 100], as OpenAI sends them
    seed: Optional[int] = None
    min_p: Optional[float] = None
    guided_choice: Optional[List[str]] = None  # vLLM's structured output: the text is one of these strings
    guided_regex: Optional[str] = None         # ... or fully matches this pattern (runtime/guide.py from_regex)
    user: Optional[str] = None
    logprobs: Optional[bool] = False
    top_logprobs: Optional[int] = None


class CompletionRequest(_Wire):
    model: str
    prompt: Union[str, List[str]]
    temperature: Optional[float] = 0.7
    top_p: Optional[float] = 1.0
    top_k: Optional[int] = 1
    n: Optional[int] = 1
    max_tokens: Optional[int] = 16
    stop: Optional[Union[str, List[str]]] = None
    stream: Optional[bool] = False
    echo: Optional[bool] = False
    repetition_penalty: Optional[float] = 1.0
    presence_penalty: Optional[float] = 0.0
    frequency_penalty: Optional[float] = 0.0
    logit_bias: Optional[Dict[str, float]] = None  # token-id strings -> [-100, 100], as OpenAI sends them
    seed: Optional[int] = None
    min_p: Optional[float] = None
    guided_choice: Optional[List[str]] = None  # vLLM's structured output: the text is one of these strings
    guided_regex: Optional[str] = None         # ... or fully matches this pattern (runtime/guide.py from_regex)
    user: Optional[str] = None
    logprobs: Optional[int] = None
    prompt_logprobs: Optional[int] = None  # 0..20: score the PROMPT's tokens (choices[i].prompt_logprobs)


def _error(status, message):
    """{"object": "error", "message", "code"} with the HTTP status as the code (textchat_api.py:104-106)."""
    return JSONResponse({"object": "error", "message": message, "code": int(status)}, status_code=int(status))


MAX_N = 8           # completions per request
MAX_TOKENS = 8192   # new tokens per completion
MAX_LOGIT_BIAS = 300  # logit_bias entries per request (OpenAI's bound)


def _vocab_size(bot):
    """ids the model scores: the engine's vocabulary, else the tokenizer's length, else unknown (None)"""
    cfg = getattr(getattr(bot, "engine", None), "cfg", None)
    if cfg is not None:
        return int(cfg.vocab)
    tok = getattr(bot, "tokenizer", None)
    return len(tok) if hasattr(tok, "__len__") else None


def _check_sampler_controls(req):
    """presence / frequency penalty, logit_bias and min_p: OpenAI's ranges, the file's message style."""
    for name in ("presence_penalty", "frequency_penalty"):
        v = getattr(req, name)
        if v is not None and not v >= -2:  # (a NaN fails the first test)
            return "%s is less than the minimum of -2 - '%s'" % (v, name)
        if v is not None and v > 2:
            return "%s is greater than the maximum of 2 - '%s'" % (v, name)
    if req.min_p is not None and not 0 <= req.min_p <= 1:
        return "%s is outside [0, 1] - 'min_p'" % req.min_p
    bias = req.logit_bias or {}
    if len(bias) > MAX_LOGIT_BIAS:
        return "%s is greater than the maximum of %d - 'logit_bias' entries" % (len(bias), MAX_LOGIT_BIAS)
    vocab = _vocab_size(router.get_chatbot()) if bias else None
    for key, v in bias.items():
        try:
            tid = int(key)
        except (TypeError, ValueError):
            return "%r is not a token id - 'logit_bias'" % (key,)
        if str(tid) != str(key).strip() or tid < 0 or (vocab is not None and tid >= vocab):
            return "%r is not a token id of this model - 'logit_bias'" % (key,)
        if not -100 <= v <= 100:
            return "%s is outside [-100, 100] - 'logit_bias'" % v
    return None


def _check_guided(req):
    """guided_choice / guided_regex: one of the two, and a pattern the guide's builder takes (its message otherwise)."""
    if req.guided_choice is None and req.guided_regex is None:
        return None
    if req.guided_choice is not None and req.guided_regex is not None:
        return "guided_choice and guided_regex cannot be used together"
    if req.guided_choice is not None and (not req.guided_choice or not all(req.guided_choice)):
        return "guided_choice is a non-empty list of non-empty strings"
    try:
        if req.guided_regex is not None:
            from ....runtime.guide import check_regex

            check_regex(req.guided_regex)
        build = getattr(router.get_chatbot(), "request_guide", None)
        if build is not None:  # over the model's own vocabulary (kept per pattern: the request reuses it)
            build(GenerationConfig(guided_choice=req.guided_choice, guided_regex=req.guided_regex))
    except ValueError as e:
        return "%s - '%s'" % (e, "guided_regex" if req.guided_regex is not None else "guided_choice")
    return None


def _check_ranges(req):
    """Parameter ranges of textchat_api.py:56-102, same messages."""
    if req.max_tokens is not None and req.max_tokens <= 0:
        return "%s is less than the minimum of 1 - 'max_tokens'" % req.max_tokens
    if req.n is not None and req.n <= 0:
        return "%s is less than the minimum of 1 - 'n'" % req.n
    # one engine serves every request in turn: bound what a single request can make the others wait for
    if req.n is not None and req.n > MAX_N:
        return "%s is greater than the maximum of %d - 'n'" % (req.n, MAX_N)
    if req.max_tokens is not None and req.max_tokens > MAX_TOKENS:
        return "%s is greater than the maximum of %d - 'max_tokens'" % (req.max_tokens, MAX_TOKENS)
    if req.temperature is not None and req.temperature < 0:
        return "%s is less than the minimum of 0 - 'temperature'" % req.temperature
    if req.temperature is not None and req.temperature > 2:
        return "%s is greater than the maximum of 2 - 'temperature'" % req.temperature
    if req.top_p is not None and not 0 <= req.top_p <= 1:
        return "%s is outside [0, 1] - 'top_p'" % req.top_p
    if req.top_k is not None and -1 < req.top_k < 1:
        return "%s is out of Range. Either set top_k to -1 or >=1." % req.top_k
    return _check_sampler_controls(req) or _check_guided(req) or _check_logprobs(req)


def _wanted_logprobs(req):
    """How many alternatives per token the request asks for (None = no log-probabilities): the chat route's
    `logprobs: true` + `top_logprobs: 0..20`, the completions route's `logprobs: 0..5`."""
    if isinstance(req, ChatCompletionRequest):
        return int(req.top_logprobs or 0) if req.logprobs else None
    return req.logprobs


def _check_logprobs(req):
    if isinstance(req, ChatCompletionRequest):
        if req.top_logprobs is not None and not 0 <= req.top_logprobs <= 20:
            return "%s is outside [0, 20] - 'top_logprobs'" % req.top_logprobs
        if req.top_logprobs is not None and not req.logprobs:
            return "'top_logprobs' needs 'logprobs' to be true"
    elif req.logprobs is not None and not 0 <= req.logprobs <= 5:
        return "%s is outside [0, 5] - 'logprobs'" % req.logprobs
    if _wanted_logprobs(req) is not None and req.stream:
        return "QBits: logprobs are not available on streamed responses"
    n_prompt = getattr(req, "prompt_logprobs", None)  # the completions route only
    if n_prompt is not None:
        if not 0 <= n_prompt <= 20:
            return "%s is outside [0, 20] - 'prompt_logprobs'" % n_prompt
        if req.stream:
            return "QBits: prompt_logprobs are not available on streamed responses"
        if not hasattr(router.get_chatbot(), "score_prompt"):
            return "QBits: this model cannot score a prompt - 'prompt_logprobs'"
    return None


def _token_bytes(token):
    return list(token.encode("utf-8"))


def _chat_logprobs(entries, n_top):
    """`choices[i].logprobs` of a chat completion from BaseModel.last_logprobs entries."""
    return {"content": [{"token": e["token"], "logprob": e["logprob"], "bytes": _token_bytes(e["token"]),
                         "top_logprobs": [{"token": s, "logprob": lp, "bytes": _token_bytes(s)}
                                          for _i, s, lp in e["top"][:n_top]]} for e in entries]}


def _completion_logprobs(entries, n_top, shift=0):
    """`choices[i].logprobs` of a plain completion; `shift` = length of an echoed prompt in front of the text."""
    return {"tokens": [e["token"] for e in entries], "token_logprobs": [e["logprob"] for e in entries],
            "top_logprobs": [{s: lp for _i, s, lp in e["top"][:n_top]} for e in entries],
            "text_offset": [e["text_offset"] + shift for e in entries]}


def _prompt_logprobs(entries, n_top):
    """`choices[i].prompt_logprobs`: the legacy completions object over the PROMPT's tokens (BaseModel.score_prompt
    entries); the first token has nothing in front of it, so its `token_logprobs` / `top_logprobs` are null."""
    return {"tokens": [e["token"] for e in entries], "token_logprobs": [e["logprob"] for e in entries],
            "top_logprobs": [None if e["logprob"] is None else {s: lp for _i, s, lp in e["top"][:n_top]}
                             for e in entries],
            "text_offset": [e["text_offset"] for e in entries]}


class TextChatAPIRouter(APIRouter):
    """`router.set_chatbot(chatbot)` then include the router in a FastAPI app (reference :374-390)."""

    def __init__(self):
        super().__init__()
        self.chatbot = None
        self._gpu = threading.Lock()  # one engine, one request at a time

    def set_chatbot(self, chatbot, use_deepspeed=False, world_size=1, host="0.0.0.0", port=80):
        if use_deepspeed:
            raise NotImplementedError("QBits: the DeepSpeed worker fan-out is not part of the MI355X path "
                                      "(tensor parallelism runs inside the engine)")
        self.chatbot, self.world_size, self.host, self.port = chatbot, world_size, host, port

    def get_chatbot(self):
        if self.chatbot is None:
            raise RuntimeError("Chatbot instance has not been set.")
        return self.chatbot

    # ---- request -> prompt / generation config -----------------------------------------------------------------
    def build_prompt(self, messages):
        """OpenAI messages -> the model family's prompt through its conversation template (reference
        get_generation_parameters :125-199): system -> system message, user / assistant turns in order, then an
        open assistant turn. A plain string is the prompt as it stands."""
        if isinstance(messages, str):
            return messages
        conv = self.get_chatbot().conv_template.copy()
        conv.messages = []
        for m in messages:
            role, content = m.get("role"), m.get("content")
            if isinstance(content, list):  # multimodal form: keep the text parts
                content = "\n".join(p.get("text", "") for p in content if p.get("type") == "text")
            if role == "system":
                conv.system_message = content
            elif role == "user":
                conv.append_message(conv.roles[0], content)
            elif role == "assistant":
                conv.append_message(conv.roles[1], content)
            else:
                raise ValueError("Unknown role: %s" % role)
        conv.append_message(conv.roles[1], None)
        return conv.get_prompt()

    @staticmethod
    def generation_config(req, default_max_tokens):
        greedy = not req.temperature or req.top_k == 1
        bias = {int(k): float(v) for k, v in (req.logit_bias or {}).items()}
        return GenerationConfig(temperature=req.temperature if req.temperature else 1.0, top_p=req.top_p,
                                top_k=req.top_k if req.top_k and req.top_k > 0 else 0,
                                repetition_penalty=req.repetition_penalty or 1.0,
                                max_new_tokens=req.max_tokens or default_max_tokens, do_sample=not greedy,
                                task="chat", presence_penalty=req.presence_penalty or 0.0,
                                frequency_penalty=req.frequency_penalty or 0.0, min_p=req.min_p or 0.0,
                                logit_bias=bias or None, seed=req.seed, guided_choice=req.guided_choice or None,
                                guided_regex=req.guided_regex)

    @staticmethod
    def _stops(req, conv=None):
        stops = [req.stop] if isinstance(req.stop, str) else list(req.stop or [])
        return [s for s in stops if s]

    def _count(self, text):
        tok = getattr(self.get_chatbot(), "tokenizer", None)
        return len(tok(text).input_ids) if tok is not None and text else 0

    # ---- generation ------------------------------------------------------------------------------------------------
    def _generate(self, prompt, config, stops):
        """-> (text, finish_reason)."""
        return self._generate_logprobs(prompt, config, stops)[:2]

    def _generate_logprobs(self, prompt, config, stops):
        """-> (text, finish_reason, the chatbot's last_logprobs entries of the kept text or None). The entries are read
        under the lock the generation ran under; a stop string keeps the tokens that start before the cut."""
        with self._gpu:
            text = self.get_chatbot().predict(query=prompt, config=config)
            entries = None
            if getattr(config, "logprobs", None) is not None:
                entries = list(getattr(self.get_chatbot(), "last_logprobs", None) or [])
        cut = min([text.find(s) for s in stops if s in text], default=-1)
        if cut >= 0:
            if entries is not None:
                entries = [e for e in entries if e["text_offset"] < cut]
            return text[:cut], "stop", entries
        return text, ("length" if self._count(text) >= config.max_new_tokens else "stop"), entries

    def _score_prompt(self, prompt, n_top):
        """BaseModel.score_prompt under the engine lock."""
        with self._gpu:
            return self.get_chatbot().score_prompt(prompt, n_top)

    def _stream(self, prompt, config, stops):
        """Text pieces until a stop string shows up (the piece is cut there). The generation itself runs in a worker
        thread that holds the engine lock only while it generates and hands pieces over a queue: a slow or vanished
        client (this generator suspended between yields, or never resumed) cannot keep the one engine locked."""
        import queue
        import threading

        # unbounded: the generation is already bounded by max_tokens, so the worker never blocks on a slow client and the
        # engine lock is held for the generation only; `done` and an exception always get through
        pieces = queue.Queue()
        gone = threading.Event()  # the consumer stopped listening (disconnect, stop string, generator closed)
        done = object()

        def work():
            try:
                with self._gpu:
                    gen, _link = self.get_chatbot().predict_stream(query=prompt, config=config)
                    if not isinstance(gen, types.GeneratorType):
                        gen = (gen,)
                    for piece in gen:
                        if gone.is_set():
                            break
                        pieces.put(piece)
                    if hasattr(gen, "close"):
                        gen.close()
                pieces.put(done)
            except BaseException as ex:  # surfaced on the consumer side
                pieces.put(ex)

        worker = threading.Thread(target=work, daemon=True)
        worker.start()
        seen = ""
        try:
            while True:
                try:
                    piece = pieces.get(timeout=1.0)
                except queue.Empty:
                    if worker.is_alive():
                        continue
                    try:  # the worker is gone: whatever it left is already in the queue
                        piece = pieces.get_nowait()
                    except queue.Empty:
                        return
                if piece is done:
                    return
                if isinstance(piece, BaseException):
                    raise piece
                if not isinstance(piece, str) or not piece:
                    continue
                seen += piece
                cut = min([seen.find(s) for s in stops if s in seen], default=-1)
                if cut >= 0:
                    keep = piece[:max(0, len(piece) - (len(seen) - cut))]
                    if keep:
                        yield keep
                    return
                yield piece
        finally:
            gone.set()


router = TextChatAPIRouter()


def _models_payload():
    name = router.get_chatbot().model_name
    now = int(time.time())
    return {"object": "list", "data": [{"id": name, "object": "model", "created": now, "owned_by": "neuralchat",
                                        "root": name, "parent": None, "permission": []}]}


@router.post("/v1/models")
async def show_available_models():
    """One model per server, as in the reference (:464-475, which answers POST)."""
    return _models_payload()


@router.get("/v1/models")
async def list_models():
    return _models_payload()


@router.get("/health")
async def health() -> Response:
    return Response(status_code=200)


def _validate(req):
    if req.model not in router.get_chatbot().model_name:  # substring match, textchat_api.py:108-115
        return _error(404, "The model `%s` does not exist." % req.model)
    bad = _check_ranges(req)
    return _error(400, bad) if bad else None


def _sse(obj):
    return "data: %s\n\n" % json.dumps(obj, ensure_ascii=False)


@router.post("/v1/chat/completions")
async def create_chat_completion(request: ChatCompletionRequest):
    """https://platform.openai.com/docs/api-reference/chat/create, as far as the reference implements it (:482-600)."""
    err = _validate(request)
    if err is not None:
        return err
    try:
        prompt = router.build_prompt(request.messages)
    except ValueError as e:
        return _error(400, str(e))
    config = router.generation_config(request, 512)
    n_top = config.logprobs = _wanted_logprobs(request)
    stops = router._stops(request)
    rid, created = "chatcmpl-" + uuid.uuid4().hex[:22], int(time.time())
    if request.stream:
        def events():
            head = {"id": rid, "object": "chat.completion.chunk", "created": created, "model": request.model}
            for i in range(request.n or 1):
                yield _sse(dict(head, choices=[{"index": i, "delta": {"role": "assistant"}, "finish_reason": None}]))
                try:
                    for piece in router._stream(prompt, config, stops):
                        yield _sse(dict(head, choices=[{"index": i, "delta": {"content": piece},
                                                        "finish_reason": None}]))
                except Exception as e:  # the reference's in-band error frame (:241-244)
                    yield _sse({"text": str(e), "error_code": 500})
                    yield "data: [DONE]\n\n"
                    return
                yield _sse(dict(head, choices=[{"index": i, "delta": {}, "finish_reason": "stop"}]))
            yield "data: [DONE]\n\n"

        return StreamingResponse(events(), media_type="text/event-stream")
    choices, n_out = [], 0
    try:
        for i in range(request.n or 1):
            text, why, entries = await run_in_threadpool(router._generate_logprobs, prompt, config, stops)
            choices.append({"index": i, "message": {"role": "assistant", "content": text}, "finish_reason": why})
            if entries is not None:
                choices[-1]["logprobs"] = _chat_logprobs(entries, n_top)
            n_out += router._count(text)
    except Exception as e:
        return _error(500, str(e))
    n_in = router._count(prompt) * (request.n or 1)
    return {"id": rid, "object": "chat.completion", "created": created, "model": request.model, "choices": choices,
            "usage": {"prompt_tokens": n_in, "total_tokens": n_in + n_out, "completion_tokens": n_out}}


@router.post("/v1/completions")
async def create_completion(request: CompletionRequest):
    """Plain completions (:603-713): every prompt x n, no chat template."""
    err = _validate(request)
    if err is not None:
        return err
    prompts = [request.prompt] if isinstance(request.prompt, str) else list(request.prompt)
    config = router.generation_config(request, 16)
    n_top = config.logprobs = _wanted_logprobs(request)
    stops = router._stops(request)
    rid, created = "cmpl-" + uuid.uuid4().hex[:22], int(time.time())
    if request.stream:
        def events():
            head = {"id": rid, "object": "text_completion", "created": created, "model": request.model}
            idx = 0
            for p in prompts:
                for _ in range(request.n or 1):
                    if request.echo:
                        yield _sse(dict(head, choices=[{"index": idx, "text": p, "logprobs": None,
                                                        "finish_reason": None}]))
                    for piece in router._stream(p, config, stops):
                        yield _sse(dict(head, choices=[{"index": idx, "text": piece, "logprobs": None,
                                                        "finish_reason": None}]))
                    yield _sse(dict(head, choices=[{"index": idx, "text": "", "logprobs": None,
                                                    "finish_reason": "stop"}]))
                    idx += 1
            yield "data: [DONE]\n\n"

        return StreamingResponse(events(), media_type="text/event-stream")
    choices, n_in, n_out = [], 0, 0
    try:
        for p in prompts:
            scored = None  # once per prompt, shared by its n choices
            if request.prompt_logprobs is not None:
                scored = _prompt_logprobs(await run_in_threadpool(router._score_prompt, p, request.prompt_logprobs),
                                          request.prompt_logprobs)
            for _ in range(request.n or 1):
                text, why, entries = await run_in_threadpool(router._generate_logprobs, p, config, stops)
                lps = None if entries is None else _completion_logprobs(entries, n_top, len(p) if request.echo else 0)
                choices.append({"index": len(choices), "text": (p + text) if request.echo else text, "logprobs": lps,
                                "finish_reason": why})
                if scored is not None:
                    choices[-1]["prompt_logprobs"] = scored
                n_in += router._count(p)
                n_out += router._count(text)
    except Exception as e:
        return _error(500, str(e))
    return {"id": rid, "object": "text_completion", "created": created, "model": request.model, "choices": choices,
            "usage": {"prompt_tokens": n_in, "total_tokens": n_in + n_out, "completion_tokens": n_out}}
