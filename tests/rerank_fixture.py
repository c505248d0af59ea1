"""What the decoder-reranker tests share: the prompt definition restated, the test tokenizer (tests/golden/bpe_qwen2_tokenizer.json
with `yes`, `no`, `<think>` and `</think>` appended as added tokens inside the 720-token vocabulary of the Chat fixture), and the
seeds of the end-to-end case."""
from __future__ import annotations

import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HEAD = ("<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct provided. Note that the "
        "answer can only be \"yes\" or \"no\".<|im_end|>\n<|im_start|>user\n")
TAIL = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
INSTRUCTION = "Given a web search query, retrieve relevant passages that answer the query"

YES, NO, THINK, END_THINK = 707, 708, 709, 710      # behind the golden's added tokens 700 .. 706
VOCAB = 720


def body(query: str, document, instruction=None) -> str:
    """The user turn; document None: up to and including "<Document>: "."""
    return f"<Instruct>: {INSTRUCTION if instruction is None else instruction}\n<Query>: {query}\n<Document>: {document or ''}"


def write_tokenizer(path: str, words=("yes", "no", "<think>", "</think>")) -> str:
    j = json.load(open(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json")))
    ids = {"yes": YES, "no": NO, "<think>": THINK, "</think>": END_THINK}
    for w in words:
        # (single_word: "no" inside "Note" or "know" stays ordinary text)
        j["added_tokens"].append({"id": ids[w], "content": w, "single_word": True, "lstrip": False, "rstrip": False, "normalized": False,
                                  "special": False})
    with open(path, "w") as f:
        json.dump(j, f)
    return path


# The end-to-end case: Q3_SMALL with vocab_size = VOCAB and room for the prompt (220 .. 263 tokens with this byte-level vocabulary).
# MODEL_SEED and MODEL_STD were chosen on the CPU with the float64 reference alone (tests/qwen3_ref64.py), so that the eight scores
# sigmoid(l_yes - l_no) of DOCUMENTS under QUERY and the default instruction are pairwise more than 100 x the bar (1e-4) apart --
# the closest two by 1.4e-2; seeds 0 .. 11 at std 0.05 leave two documents within 3e-3, every document ending in the same
# assistant turn -- and the GPU test asserts that margin again.  (Under OTHER_INSTRUCTION only the values are compared.)
MODEL_SEED = 8
MODEL_STD = 0.1
MAX_POSITIONS = 1024
QUERY = "Which river runs through Paris?"
DOCUMENTS = [
    "The Seine runs through Paris.",
    "Berlin lies on the Spree.",
    "A recipe for onion soup.",
    "Paris is the capital of France; the Seine crosses it from east to west.",
    "The Thames runs through London.",
    "Rivers carry water to the sea.",
    "no",
    "The Danube passes Vienna, Bratislava, Budapest and Belgrade.",
]
OTHER_INSTRUCTION = "Find the passage that names the river"
