"""CPU: every chunk geometry `pipe_chunking` can give survives the pipelined decode kernel's geometry word. A chunked launch sends its flags,
`wg_per_xcd`, `n_chunks` (less one) and `n_tiles` in ONE preloaded dword, a byte each (csrc/common.hpp `pipe_geom_word` / `pipe_geom_unpack`), and the launcher
refuses what `pipe_geom_fits` rejects -- so a geometry that does not fit would turn a launch that used to run into an error. A stand-alone
host program (no GPU call in it) walks n_tiles 1..128 and n_half 2..70000 -- 2.2 M rows, far past what the 32-bit offsets of the kernel
admit -- and checks fit and round trip for each, with every flag bit set and clear. The widest case is a sub-model of ONE tile (a landmark
list of up to 20 vertices) whose n_half is a multiple of 256: 256 chunks."""
import subprocess

from kernel_resources import CSRC, HIPCC, needs_hipcc

PROGRAM = r"""
#include "common.hpp"
#include <cstdio>
int main() {
    using namespace dad3d;
    long checked = 0;
    int widest = 0;
    for (int n_tiles = 1; n_tiles <= 128; ++n_tiles)
        for (int n_half = 2; n_half <= 70000; ++n_half) {
            int chunk_half, n_chunks, wg;
            pipe_chunking(n_tiles, n_half, &chunk_half, &n_chunks, &wg);
            if (chunk_half == 0) continue;  // not chunked: the word carries the flags alone
            if (n_tiles * n_chunks > 256 || wg > 32 || n_chunks < 2) { std::printf("pipe_chunking: %d %d -> %d %d\n", n_tiles, n_half, n_chunks, wg); return 1; }
            if (!pipe_geom_fits(wg, n_chunks, n_tiles)) { std::printf("does not fit: %d %d -> %d %d\n", n_tiles, n_half, n_chunks, wg); return 1; }
            for (unsigned flags : {0u, 0xFFu, 0x5Au, 0xA5u}) {
                const PipeGeom g = pipe_geom_unpack(pipe_geom_word(flags, wg, n_chunks, n_tiles));
                if (g.flags != flags || g.wg_per_xcd != wg || g.n_chunks != n_chunks || g.n_tiles != n_tiles) {
                    std::printf("round trip: %d %d -> %d %d flags %x\n", n_tiles, n_half, n_chunks, wg, flags);
                    return 1;
                }
            }
            if (n_chunks > widest) widest = n_chunks;
            ++checked;
        }
    const PipeGeom plain = pipe_geom_unpack(pipe_geom_word(0xFFu, 0, 1, 0));  // not chunked: one chunk, as PipeArgs says
    if (plain.flags != 0xFFu || plain.wg_per_xcd || plain.n_chunks != 1 || plain.n_tiles) return 1;
    std::printf("checked %ld widest %d\n", checked, widest);
    return 0;
}
"""


@needs_hipcc
def test_every_chunk_geometry_round_trips(tmp_path):
    src, exe = tmp_path / "geom.cpp", tmp_path / "geom"
    src.write_text(PROGRAM)
    build = subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    checked, widest = (int(x) for x in run.stdout.split()[1::2])
    assert checked > 8_000_000 and widest == 256, run.stdout  # the one-tile sub-model at n_half = 256 k is in the walk
