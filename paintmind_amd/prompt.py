"""Prompt emphasis syntax: ``a (red:1.4) barn, (blurry:0.5)`` -> fragments with weights.

``(words:1.3)`` gives the words inside the weight 1.3; text outside any parentheses has weight 1.  Parentheses nest and their
weights multiply: ``(a (b:2) c:3)`` is ``a `` and `` c`` at 3 and ``b`` at 6.  A backslash takes the next ``(``, ``)``, ``:`` or
``\\`` literally.  Every group needs its ``:number``; the number is a non-negative decimal.  What the weights mean -- and the range
they must stay in after multiplying, 0 or [2^-20, 2^20] -- is the cross-attention's business (``ops.host_weights``), not the
parser's.

``align_rows`` pairs the context rows of two prompts for prompt-to-prompt editing: pure Python over token ids.
"""

_ESCAPABLE = "():\\"


def parse_weighted(text):
    """-> [(fragment, weight), ...] in reading order, empty fragments dropped, neighbours of equal weight merged; the fragments
    joined give the prompt without its syntax.  Unbalanced parentheses, a group without ``:number`` or a weight that is no
    non-negative number raise a ValueError that names the position (0-based, in ``text``)."""
    if not isinstance(text, str):
        raise TypeError(f"parse_weighted takes a string, got {type(text).__name__}")
    out = []                 # [fragment, weight] of closed text
    stack = []               # per open group: (position of its "(", index into `out` where its fragments start)
    buf = []                 # characters of the fragment being read

    def flush():
        if buf:
            out.append(["".join(buf), 1.0])
            buf.clear()

    i, n = 0, len(text)
    while i < n:
        ch = text[i]
        if ch == "\\" and i + 1 < n and text[i + 1] in _ESCAPABLE:
            buf.append(text[i + 1])
            i += 2
        elif ch == "(":
            flush()
            stack.append((i, len(out)))
            i += 1
        elif ch == ":" and stack:
            j = i + 1
            while j < n and text[j] not in "()":
                j += 1
            if j >= n or text[j] != ")":
                raise ValueError(f"prompt weights: position {i}: ':' inside a group must be followed by a number and ')' "
                                 f"(write '\\:' for a literal colon) in {text!r}")
            num = text[i + 1:j].strip()
            try:
                w = float(num)
            except ValueError:
                w = None
            if w is None or not (w >= 0.0) or w == float("inf") or not num.replace(".", "", 1).isdigit():
                raise ValueError(f"prompt weights: position {i + 1}: {num!r} is no non-negative number in {text!r}")
            flush()
            _, start = stack.pop()
            for item in out[start:]:
                item[1] *= w
            i = j + 1
        elif ch == ")":
            if not stack:
                raise ValueError(f"prompt weights: position {i}: ')' without a '(' (write '\\)' for a literal one) in {text!r}")
            raise ValueError(f"prompt weights: position {i}: the group opened at position {stack[-1][0]} closes without ':number' "
                             f"in {text!r}")
        else:
            buf.append(ch)
            i += 1
    if stack:
        raise ValueError(f"prompt weights: position {stack[-1][0]}: '(' is never closed (write '\\(' for a literal one) in {text!r}")
    flush()
    merged = []
    for frag, w in out:
        if merged and merged[-1][1] == w:
            merged[-1] = (merged[-1][0] + frag, w)
        else:
            merged.append((frag, w))
    return merged


def strip_weights(text):
    """the prompt without its emphasis syntax"""
    return "".join(frag for frag, _ in parse_weighted(text))


def align_rows(src_ids, tgt_ids, mode="refine"):
    """Which context row of the source prompt every context row of the edited prompt takes its cross-attention from.

    src_ids, tgt_ids: the token ids of the two prompts, each ending with its end-of-sequence token (no padding).
    -> (row_map, blend): two lists as long as tgt_ids -- the source row of every target row (-1: none) and its blend, the
    arguments of ``ops.attention_control`` for one pair.

    The end-of-sequence rows pair with each other.  In front of them a longest common subsequence pairs equal tokens, blend 1; among
    the longest ones the pairing that uses the earliest source rows is taken (and, for a source row, the earliest target row).
    mode 'refine' : an unpaired target row gets -1 and blend 0 (it attends as the edited prompt says)
    mode 'replace': an unpaired target span of n rows between two paired rows (the start of the prompt counts as one) is laid over the
                    unpaired source span of m rows between the same two: its row i takes source row floor(i * m / n) of that span,
                    blend 1.  With m = 0 there is nothing to lay it over and the span is treated as in 'refine'."""
    if mode not in ("refine", "replace"):
        raise ValueError(f"align_rows: mode must be 'refine' or 'replace', not {mode!r}")
    src, tgt = list(src_ids), list(tgt_ids)
    if not src or not tgt:
        raise ValueError("align_rows: a prompt has at least its end-of-sequence token")
    ns, nt = len(src) - 1, len(tgt) - 1
    # lcs[i][j]: the length of a longest common subsequence of src[i:ns] and tgt[j:nt]
    lcs = [[0] * (nt + 1) for _ in range(ns + 1)]
    for i in range(ns - 1, -1, -1):
        for j in range(nt - 1, -1, -1):
            lcs[i][j] = lcs[i + 1][j + 1] + 1 if src[i] == tgt[j] else max(lcs[i + 1][j], lcs[i][j + 1])
    pairs, i, j = [], 0, 0
    while lcs[i][j] > 0:
        step = next((a, b) for a in range(i, ns) for b in range(j, nt) if src[a] == tgt[b] and lcs[a + 1][b + 1] + 1 == lcs[i][j])
        pairs.append(step)
        i, j = step[0] + 1, step[1] + 1
    pairs.append((ns, nt))
    row_map, blend = [-1] * (nt + 1), [0.0] * (nt + 1)
    a0, b0 = -1, -1
    for a, b in pairs:
        row_map[b], blend[b] = a, 1.0
        m, n = a - a0 - 1, b - b0 - 1
        if mode == "replace" and m > 0:
            for k in range(n):
                row_map[b0 + 1 + k], blend[b0 + 1 + k] = a0 + 1 + (k * m) // n, 1.0
        a0, b0 = a, b
    return row_map, blend
