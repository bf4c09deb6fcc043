#!/usr/bin/env python3
"""Generates vqnerf_release_amd/csrc/mc_table.h: the marching-cubes case table, from a rule instead of from memory.

    python tools/gen_mc_table.py [OUT]        (default OUT: vqnerf_release_amd/csrc/mc_table.h)

Conventions (repeated at the top of the header):
  * corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) = (x, y, z) from the cell's minimum corner and is INSIDE
    iff u[c] > threshold (strict); case = sum of (1 << c) over the inside corners;
  * edge e = 4 * axis + k runs along `axis` (0 x, 1 y, 2 z) from its low corner; k = lo + 2 * hi with (lo, hi) the low corner's offsets
    along the two other axes in increasing axis order.  Grid point (i, j, k) owns the three grid edges leaving it in +x, +y, +z.

Rule, per case:
  1. on each of the six faces walk the four corners counter-clockwise as seen from outside the cell; a crossed edge where the walk
     goes outside -> inside ENTERS, one where it goes inside -> outside EXITS (0, 1 or 2 of each);
  2. every maximal run of inside corners gives one directed segment, from the edge that enters it to the edge that exits it.  With
     four crossings (two inside corners on a diagonal: the ambiguous face) that is one segment around each inside corner: the two
     inside corners are always SEPARATED.  The choice depends on the face's four corner signs only, so the two cells that share a
     face make the same one;
  3. the segments chain into closed loops (every crossed edge lies on two faces: it enters on one and exits on the other);
  4. each loop is fan-triangulated from its lowest-numbered edge, in loop order.
A segment from an entering to an exiting edge has the inside corners on its right as seen from outside the cell, so the triangles
come out counter-clockwise as seen from the outside of the surface: their normals point from inside to outside, towards decreasing u.
The output is deterministic (no dictionaries of unordered keys, no randomness).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, 'vqnerf_release_amd', 'csrc', 'mc_table.h')


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_index(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def edge_corners(e):
    """(low corner, high corner) of edge e"""
    axis, k = divmod(e, 4)
    others = [a for a in range(3) if a != axis]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = k & 1, k >> 1
    lo = corner_index(off)
    off[axis] = 1
    return lo, corner_index(off)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def face_cycle(axis, side):
    """the four corners of the face `axis` = side, counter-clockwise as seen from outside the cell"""
    b, c = (axis + 1) % 3, (axis + 2) % 3                 # e_b x e_c = e_axis: (0,0) (1,0) (1,1) (0,1) is ccw seen from +axis
    cyc = []
    for vb, vc in ((0, 0), (1, 0), (1, 1), (0, 1)):
        off = [0, 0, 0]
        off[axis], off[b], off[c] = side, vb, vc
        cyc.append(corner_index(off))
    return cyc if side == 1 else cyc[::-1]


def face_segments(case, axis, side):
    """directed segments (edge entered -> edge exited) of one face, one per maximal run of inside corners"""
    cyc = face_cycle(axis, side)
    ins = [(case >> c) & 1 for c in cyc]
    if all(ins) or not any(ins):
        return []
    segs = []
    for i in range(4):
        if not ins[i - 1] and ins[i]:                     # the walk enters an inside run at corner i ...
            j = i
            while ins[(j + 1) % 4]:
                j += 1                                    # ... which ends at corner j
            enter = EDGE_OF[frozenset((cyc[i - 1], cyc[i]))]
            leave = EDGE_OF[frozenset((cyc[j % 4], cyc[(j + 1) % 4]))]
            segs.append((enter, leave))
    return segs


def case_triangles(case):
    nxt = {}
    for axis in range(3):
        for side in range(2):
            for a, b in face_segments(case, axis, side):
                assert a not in nxt, (case, a)
                nxt[a] = b
    crossed = [e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1]
    assert sorted(nxt) == crossed and sorted(nxt.values()) == crossed, case
    tris, seen = [], set()
    for start in crossed:                                 # increasing: every loop starts at its lowest-numbered edge
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, case
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    mask = sum(1 << e for e in crossed)
    return tris, mask


def render():
    cases = [case_triangles(c) for c in range(256)]
    most = max(len(t) for t, _ in cases)
    assert most <= 5, most
    L = []
    L.append('/* mc_table.h -- marching-cubes case table.  GENERATED by tools/gen_mc_table.py: do not edit, re-run the generator')
    L.append(' * (tests/test_mc_table.py re-generates it and compares byte for byte).')
    L.append(' *')
    L.append(' * Conventions:')
    L.append(' *  - corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) = (x, y, z) from the cell\'s minimum corner and is')
    L.append(' *    INSIDE iff u[c] > threshold (strict); case = sum of (1 << c) over the inside corners.')
    L.append(' *  - edge e = 4 * axis + k runs along axis (0 x, 1 y, 2 z) from its low corner; k = lo + 2 * hi, (lo, hi) = the low corner\'s')
    L.append(' *    offsets along the two other axes in increasing axis order:')
    for e in range(12):
        lo, hi = edge_corners(e)
        L.append(' *      edge %2d: corner %d (%d,%d,%d) -> corner %d (%d,%d,%d)' % ((e, lo) + corner_offset(lo) + (hi,) + corner_offset(hi)))
    L.append(' *    Grid point (i, j, k) owns the three grid edges leaving it in +x, +y, +z.')
    L.append(' *  - ambiguous faces (four crossings): the two inside corners are always separated, one segment around each.  The choice')
    L.append(' *    depends on the four corner signs of the face only, so the two cells that share a face agree.')
    L.append(' *  - every loop of face segments is fan-triangulated from its lowest-numbered edge; triangles are counter-clockwise seen')
    L.append(' *    from outside the surface: normals point from inside to outside, towards decreasing u.')
    L.append(' *')
    L.append(' * vqn_mc_tri_count[case]: triangles of the case (0..%d).  vqn_mc_tri_edges[case][3 t + v]: edge that carries vertex v of' % most)
    L.append(' * triangle t (-1 past the end).  vqn_mc_edge_mask[case]: bit e set iff edge e is crossed.')
    L.append(' * Define VQN_MC_TABLE_QUAL before the include to place the arrays (the kernels: __constant__); default: static. */')
    L.append('#ifndef VQN_MC_TABLE_H_')
    L.append('#define VQN_MC_TABLE_H_')
    L.append('#ifndef VQN_MC_TABLE_QUAL')
    L.append('#define VQN_MC_TABLE_QUAL static')
    L.append('#endif')
    L.append('')
    L.append('VQN_MC_TABLE_QUAL const unsigned char vqn_mc_tri_count[256] = {')
    for r in range(0, 256, 32):
        L.append('  ' + ' '.join('%d,' % len(cases[c][0]) for c in range(r, r + 32)))
    L.append('};')
    L.append('')
    L.append('VQN_MC_TABLE_QUAL const unsigned short vqn_mc_edge_mask[256] = {')
    for r in range(0, 256, 8):
        L.append('  ' + ' '.join('0x%03x,' % cases[c][1] for c in range(r, r + 8)))
    L.append('};')
    L.append('')
    L.append('VQN_MC_TABLE_QUAL const signed char vqn_mc_tri_edges[256][15] = {')
    for c in range(256):
        flat = [e for t in cases[c][0] for e in t]
        flat += [-1] * (15 - len(flat))
        L.append('  {' + ', '.join('%2d' % e for e in flat) + '},  /* case %3d */' % c)
    L.append('};')
    L.append('')
    L.append('#endif /* VQN_MC_TABLE_H_ */')
    return '\n'.join(L) + '\n'


def main(argv):
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    with open(out, 'w') as f:
        f.write(render())


if __name__ == '__main__':
    main(sys.argv)
