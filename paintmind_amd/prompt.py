"""Prompt emphasis syntax: ``a (red:1.4) barn, (blurry:0.5)`` -> fragments with weights.

``(words:1.3)`` gives the words inside the weight 1.3; text outside any parentheses has weight 1.  Parentheses nest and their
weights multiply: ``(a (b:2) c:3)`` is ``a `` and `` c`` at 3 and ``b`` at 6.  A backslash takes the next ``(``, ``)``, ``:`` or
``\\`` literally.  Every group needs its ``:number``; the number is a non-negative decimal.  What the weights mean -- and the range
they must stay in after multiplying, 0 or [2^-20, 2^20] -- is the cross-attention's business (``ops.host_weights``), not the
parser's.
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
