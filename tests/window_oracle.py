"""The window rule over lists of ints, stated once and on its own (nothing of the product is imported), and the shape lists
the window tests share.  tests/test_window_inputs.py ties `windows` to the reference's restatement and checks that the
lists hold the cases they are named for; tests/test_gpu_windows.py compares the GPU with it."""
import numpy as np


def windows(body, L, s, bos, eos, pad):
    """[(row, mask, start, n_real)] of one body: room = L - 2 tokens a window, the next one starts step = room - s later."""
    room, step, T = L - 2, L - 2 - s, len(body)
    n_win = 1 if T <= room else 1 + -(-(T - room) // step)
    out = []
    for j in range(n_win):
        chunk = list(body[j * step:min(j * step + room, T)])
        row = [bos] + chunk + [eos] + [pad] * (room - len(chunk))
        out.append((row, [int(v != pad) for v in row], j * step, len(chunk) + 2))
    return out


def batch(bodies, L, s, bos, eos, pad):
    """`windows` over many bodies, in the arrays the product returns."""
    per = [windows(b, L, s, bos, eos, pad) for b in bodies]
    flat = [(w, d) for d, ws in enumerate(per) for w in ws]
    win_off = np.zeros(len(bodies) + 1, dtype=np.int64)
    if bodies:
        np.cumsum([len(ws) for ws in per], out=win_off[1:])
    return dict(input_ids=np.array([w[0] for w, _ in flat], dtype=np.int32).reshape(len(flat), L),
                attention_mask=np.array([w[1] for w, _ in flat], dtype=np.int32).reshape(len(flat), L),
                doc=np.array([d for _, d in flat], dtype=np.int32), start=np.array([w[2] for w, _ in flat], dtype=np.int32),
                n_real=np.array([w[3] for w, _ in flat], dtype=np.int32), win_off=win_off)


# (max_len, stride): the smallest row, strides 0 / 1 / the largest (step 1), rows of one store, of a wave's width and beyond,
# max_len % 4 of 0, 1, 2 and 3
RULE_CASES = [(3, 0), (4, 0), (4, 1), (5, 1), (7, 4), (10, 0), (10, 3), (64, 0), (64, 61), (65, 7), (256, 32), (257, 0), (512, 509)]


def edge_lengths(L, s):
    """Body lengths at the rule's edges: nothing, one token, around `room` (one window / two), around room + step (two
    windows / three; room + step + 1 leaves the last window ONE new token), and four windows."""
    room, step = L - 2, L - 2 - s
    return sorted({0, 1, room - 1, room, room + 1, room + step - 1, room + step, room + step + 1, room + 3 * step})


ALIGN_LENGTHS = list(range(41))          # successive rows of 0 .. 40 tokens: the rows start at the triangular numbers
ALIGN_CASES = [(10, 0), (10, 3), (16, 0), (16, 5)]

# words of the end-to-end texts: whole-word hits, words that split into several pieces, one word outside the vocabulary
WORDS = ["sinh_viên", "công_nghệ", "hello", "xin", "chào", "Việt_Nam", "học", "máy", "a", "và", "là", "của", "tokenization",
         "internationalization", "GPU", "2024", "thế_giới", "không", "một", "người", "trường_đại_học", "zzqxj中q", "nghiên_cứu", "!"]


def texts(n, max_words, seed):
    import random
    r = random.Random(seed)
    return [" ".join(r.choice(WORDS) for _ in range(r.randint(0, max_words))) for _ in range(n)]
