"""The prefabricated Huffman tables of the device PNG encoder (csrc/png_plan.h, csrc/png_encode.hip).

    python scripts/make_png_tables.py            prints the block that stands between the GENERATED marks of csrc/png_plan.h
    python scripts/make_png_tables.py --check    compares it with the header (tests/test_png_model.py does the same)

The device builds no table: per segment it sizes the tokens under each of these and takes the smallest.  A table is three rows of
code lengths: 288 literal / length symbols (286 and 287 have none), 30 distance symbols, and the 19 symbols of the code-length code
that the dynamic-block header is written with.  Every symbol 0 .. 285 and every distance symbol has a code, so any segment is codable
under any table; each set is complete (Kraft sum exactly 1); lengths are at most 15 (7 for the code-length code).

The symbol models, all in integer arithmetic (the same tables on every machine):
  literals   a filtered byte v is the residual s = v or v - 256, whichever is smaller in magnitude; weight (a / b) ^ |s|, a two-sided
             geometric law, at the seven widths WIDTHS
  matches    a share SHARES of the tokens: a quarter of them of length 258 (symbol 285), the rest falling by 7 / 8 per length symbol
             from 257 on; a quarter of the distances in symbol 0 (distance 1), a quarter spread over symbols 1 .. 5 (distances 2 .. 8,
             the short candidates of the matcher), half over symbols 6 .. 29 (wherever the row stride falls)
  end        one end-of-block symbol per 2048 tokens
Lengths come from the package-merge algorithm (optimal under the length limit), ties in stable order of (weight, symbol)."""
import os
import sys

WIDTHS = [(1, 2), (2, 3), (4, 5), (8, 9), (16, 17), (32, 33), (64, 65)]
SHARES = [(1, 16), (1, 2)]
TOKENS = 1 << 30                    # the mass the models are scaled to
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def limited_lengths(freqs, limit):
    """package-merge: code lengths <= limit of the symbols with freqs > 0 (0 for the others)"""
    leaves = sorted((f, i) for i, f in enumerate(freqs) if f > 0)
    n = len(leaves)
    lens = [0] * len(freqs)
    if n == 1:
        lens[leaves[0][1]] = 1
        return lens
    assert (1 << limit) >= n
    leaves = [(f, (i,)) for f, i in leaves]
    packages = leaves
    for _ in range(limit - 1):
        paired = [(packages[k][0] + packages[k + 1][0], packages[k][1] + packages[k + 1][1]) for k in range(0, len(packages) - 1, 2)]
        packages = sorted(leaves + paired, key=lambda t: t[0])
    for _, items in packages[:2 * n - 2]:
        for i in items:
            lens[i] += 1
    return lens


def spread(mass, weights):
    total = sum(weights)
    return [max(1, mass * w // total) for w in weights]


def symbol_model(width, share):
    a, b = width
    num, den = share
    matches = TOKENS * num // den
    lit_w = [(a ** min(v, 256 - v)) * (b ** (128 - min(v, 256 - v))) for v in range(256)]
    lit = spread(TOKENS - matches, lit_w)
    end = [TOKENS // 2048]
    length = spread(matches - matches // 4, [7 ** k * 8 ** (27 - k) for k in range(28)]) + [matches // 4]
    dist = [matches // 4] + spread(matches // 4, [1] * 5) + spread(matches // 2, [1] * 24)
    return lit + end + length, dist


def run_length_code(lens):
    """[(symbol, extra bits, extra value)] of the code-length alphabet for a row of NON-ZERO lengths: a length, then 16 (repeat the
    previous 3 .. 6 times) while at least three more of it follow"""
    out, i = [], 0
    while i < len(lens):
        v = lens[i]
        assert v > 0
        run = 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        out.append((v, 0, 0))
        i, run = i + 1, run - 1
        while run >= 3:
            k = min(run, 6)
            out.append((16, 2, k - 3))
            i, run = i + k, run - k
    return out


def table(width, share):
    litlen, dist = symbol_model(width, share)
    lit_lens = limited_lengths(litlen, 15) + [0, 0]
    dist_lens = limited_lengths(dist, 15)
    freq = [0] * 19
    for s, _, _ in run_length_code(lit_lens[:286] + dist_lens):
        freq[s] += 1
    return lit_lens, dist_lens, limited_lengths(freq, 7)


def tables():
    """[(288 literal / length code lengths, 30 distance code lengths, 19 code-length code lengths)], width-major"""
    return [table(w, s) for w in WIDTHS for s in SHARES]


def generated_block():
    tabs = tables()
    rows = lambda k: ',\n'.join('    {' + ', '.join(str(v) for v in t[k]) + '}' for t in tabs)
    return (f'constexpr int kPngTables = {len(tabs)};\n'
            f'static constexpr uint8_t kPngLitLens[kPngTables][288] = {{\n{rows(0)}}};\n'
            f'static constexpr uint8_t kPngDistLens[kPngTables][30] = {{\n{rows(1)}}};\n'
            f'static constexpr uint8_t kPngClLens[kPngTables][19] = {{\n{rows(2)}}};\n')


def header_block():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'vqnerf_release_amd', 'csrc', 'png_plan.h')).read()
    return src.split('// ---- GENERATED by scripts/make_png_tables.py: begin\n')[1].split('// ---- GENERATED: end')[0]


if __name__ == '__main__':
    if '--check' in sys.argv:
        ok = header_block() == generated_block()
        print('csrc/png_plan.h holds the generated tables' if ok else 'csrc/png_plan.h differs from the generated tables')
        sys.exit(0 if ok else 1)
    sys.stdout.write(generated_block())
