// nonrigid_gn_index_check.cpp -- host check of csrc/nonrigid_gn_index.h, the only place the Gauss-Newton non-rigid ICP kernels
// (csrc/nonrigid_gn.hip) compute an index.  Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/nonrigid_gn_index_check.cpp \
//         -o /tmp/nonrigid_gn_index_check && /tmp/nonrigid_gn_index_check
//
// It walks, as the kernels do and on a real allocation of exactly the carved size (AddressSanitizer guards its end):
//   * the workspace carve: regions ascending, disjoint, 256-byte aligned, the lists' carve at offset 0, every region written end to end;
//   * the order of the unknowns: nrg_unknown is a bijection of (node, component) onto [0, 6 M), rotations first;
//   * the assembly: every (row of node n, column of partner m) lands inside pair p's leading 6 M corner of its slot of ld x ld doubles,
//     row block n is written by node n alone, and the right-hand side inside the pair's ld doubles;
//   * the blocked factorisation at step k: the diagonal tile, the panel's row blocks and the trailing update's grid of (nb - k - 1)^2
//     workgroups touch every element of the lower triangle behind column block k exactly once each, nothing above the diagonal and nothing
//     outside the leading n x n corner -- for a ragged batch where the grid is sized by the largest system;
//   * the substitution: every row of every block is visited once per pass, the rows below (forward) and above (backward) once per block;
// over the sizes of the GPU test: n = 1, 6, 63, 64, 65, 197 alone and 65 | 6 | 197 in one batch; M = 1, 2, 10, 11, 25, 32, 40, 67 and the
// batch 1 | 25 | 10; the capacity M = 1024 for the carve and the unknowns (its 302 MB matrix is not allocated).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nonrigid_gn_index.h"

using namespace dr;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static long long g_elems = 0, g_tiles = 0;

static void walk_unknowns(int M) {
    std::vector<int> seen(6 * (size_t)M, 0);
    for (int n = 0; n < M; ++n)
        for (int i = 0; i < 6; ++i) {
            const int u = nrg_unknown(M, n, i);
            CHECK(u >= 0 && u < 6 * M);
            CHECK(i < 3 ? u < 3 * M : u >= 3 * M);
            ++seen[u];
        }
    for (int v : seen) CHECK(v == 1);
}

static void walk_carve(const std::vector<int>& Ms, int n_corr, int n_edges, int K, bool touch) {
    const int P = (int)Ms.size();
    int n_nodes = 0, max_nodes = 0;
    for (int m : Ms) { n_nodes += m; max_nodes = m > max_nodes ? m : max_nodes; }
    const NrGnCarve c = nrg_carve(P, n_corr, n_nodes, n_edges, K, max_nodes);
    const NrSolveCarve l = nr_solve_carve(P, n_corr, n_nodes, n_edges, K);
    CHECK(c.lists.bytes == l.bytes && c.lists.in_adj == l.in_adj && c.lists.resid == 0);
    const size_t starts[] = {c.n6, c.rot, c.trn, c.jac, c.b, c.A, c.bytes};
    const size_t sizes[] = {(size_t)P * 4, (size_t)n_nodes * 36, (size_t)n_nodes * 12, (size_t)n_corr * K * 32, (size_t)P * c.ld * 8,
                            (size_t)P * c.ld * c.ld * 8};
    CHECK(c.n6 == l.bytes && c.ld == 6 * max_nodes);
    for (int r = 0; r < 6; ++r) {
        CHECK(starts[r] % 256 == 0);
        CHECK(starts[r] + sizes[r] <= starts[r + 1]);
    }
    if (!touch) return;
    std::vector<unsigned char> ws(c.bytes);                 // exact size: ASan guards the end
    for (int r = 0; r < 6; ++r) std::memset(ws.data() + starts[r], r + 1, sizes[r]);
    // the assembly's writes: row block n of pair p, against every partner m, and the right-hand side
    double* A = (double*)(ws.data() + c.A);
    double* b = (double*)(ws.data() + c.b);
    std::memset(A, 0, sizes[5]);
    std::memset(b, 0, sizes[4]);
    for (int p = 0; p < P; ++p) {
        const int M = Ms[p];
        for (int n = 0; n < M; ++n)
            for (int i = 0; i < 6; ++i) {
                const int row = nrg_unknown(M, n, i);
                for (int m = 0; m < M; ++m)
                    for (int j = 0; j < 6; ++j) {
                        const size_t at = nrg_elem(p, c.ld, row, 0) + (size_t)nrg_unknown(M, m, j);
                        CHECK(at == nrg_elem(p, c.ld, row, nrg_unknown(M, m, j)));
                        CHECK(at < (size_t)P * c.ld * c.ld);
                        A[at] += 1.0;
                        ++g_elems;
                    }
                b[nrg_rhs(p, c.ld, row)] += 1.0;
            }
        for (int r = 0; r < c.ld; ++r)
            for (int col = 0; col < c.ld; ++col)
                CHECK(A[nrg_elem(p, c.ld, r, col)] == ((r < 6 * M && col < 6 * M) ? 1.0 : 0.0));
        for (int r = 0; r < c.ld; ++r) CHECK(b[nrg_rhs(p, c.ld, r)] == (r < 6 * M ? 1.0 : 0.0));
    }
}

// the factorisation's and the substitution's accesses on a batch of systems in slots of n_max x n_max
static void walk_factor(const std::vector<int>& ns) {
    const int P = (int)ns.size();
    int n_max = 0;
    for (int n : ns) n_max = n > n_max ? n : n_max;
    CHECK(n_max <= NRG_MAX_N);
    const int ld = n_max, nb = nrg_blocks(n_max);
    std::vector<int> hit((size_t)P * ld * ld);              // exact size
    for (int k = 0; k < nb; ++k) {
        std::fill(hit.begin(), hit.end(), 0);
        for (int p = 0; p < P; ++p) {
            const int n = ns[p], bw = nrg_block_rows(n, k), k0 = k * NRG_B;
            CHECK(bw >= 0 && bw <= NRG_B && (bw == 0 || k0 + bw <= n));
            // diagonal tile
            for (int r = 0; r < bw; ++r)
                for (int c = 0; c <= r; ++c) ++hit[nrg_elem(p, ld, k0 + r, k0 + c)];
            // panel: workgroup x, one row per thread, NRG_B columns of block k (full whenever a row block lies below it)
            for (int x = 0; x < nb - k - 1; ++x) {
                const int bi = k + 1 + x, rows = nrg_block_rows(n, bi);
                if (rows <= 0) continue;
                CHECK(bw == NRG_B);
                for (int r = 0; r < rows; ++r)
                    for (int j = 0; j < NRG_B; ++j) ++hit[nrg_elem(p, ld, bi * NRG_B + r, k0 + j)];
            }
            // trailing update: the grid's square of workgroups, those on and below the diagonal work
            for (int x = 0; x < nb - k - 1; ++x)
                for (int y = 0; y < nb - k - 1; ++y) {
                    int bi, bj;
                    if (!nrg_update_tile(n, k, x, y, bi, bj)) continue;
                    ++g_tiles;
                    const int ri = nrg_block_rows(n, bi), rj = nrg_block_rows(n, bj);
                    CHECK(ri > 0 && rj == NRG_B - (bj == bi ? NRG_B - ri : 0));
                    for (int r = 0; r < NRG_B; ++r)
                        for (int c = 0; c < NRG_B; ++c) {
                            const int R = bi * NRG_B + r, Cc = bj * NRG_B + c;
                            if (r < ri && c < rj && Cc <= R) ++hit[nrg_elem(p, ld, R, Cc)];
                        }
                }
            // everything in the lower triangle from column block k on, inside the corner, exactly once; nothing else
            for (int r = 0; r < ld; ++r)
                for (int c = 0; c < ld; ++c) {
                    const bool want = r < n && c <= r && c >= k0;
                    CHECK(hit[nrg_elem(p, ld, r, c)] == (want ? 1 : 0));
                }
        }
    }
    // substitution: per pass every row solved once in its block, and updated once by every block before (forward) / behind (backward) it
    for (int p = 0; p < P; ++p) {
        const int n = ns[p], nbp = nrg_blocks(n);
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<int> solved(n > 0 ? n : 0, 0), updated(n > 0 ? n : 0, 0);
            for (int step = 0; step < nbp; ++step) {
                const int kb = pass == 0 ? step : nbp - 1 - step, k0 = kb * NRG_B, bw = nrg_block_rows(n, kb);
                for (int t = 0; t < bw; ++t) ++solved[k0 + t];
                if (pass == 0)
                    for (int i = k0 + bw; i < n; ++i) { CHECK(nrg_elem(p, ld, i, k0 + bw - 1) < hit.size()); ++updated[i]; }
                else
                    for (int i = 0; i < k0; ++i) { CHECK(nrg_elem(p, ld, k0 + bw - 1, i) < hit.size()); ++updated[i]; }
            }
            for (int i = 0; i < n; ++i) {
                CHECK(solved[i] == 1);
                CHECK(updated[i] == (pass == 0 ? i / NRG_B : nbp - 1 - i / NRG_B));
                CHECK(nrg_rhs(p, ld, i) < (size_t)P * ld);
            }
        }
    }
}

int main() {
    CHECK(NRG_MAX_NODES >= nr_node_capacity());             // at least the Adam solver's capacity
    CHECK(3 * (NRG_MAX_NODES + 1) * 4 <= 64 * 1024);         // the set-up pass's static LDS scratch: three arrays of M + 1 ints
    CHECK(NRG_B * (NRG_B + 1) * 8 + NRG_B * 8 <= 64 * 1024);   // the diagonal tile (64 x 65) and the block's 64 solved values: diag, substitution
    CHECK(NRG_B * (NRG_B + 1) / 2 * 8 + NRG_B * NRG_B * 8 <= 64 * 1024);   // the panel: L_kk packed by rows and 64 rows of 64 columns
    CHECK(2 * (NRG_B / 2) * NRG_TILE_PAD * 8 <= 64 * 1024 && (NRG_TILE_PAD * 8) % 16 == 0 && NRG_TILE_PAD >= NRG_B);
    CHECK(NRG_UPDATE_T * 16 == NRG_B * NRG_B);
    for (int M : {1, 2, 10, 11, 25, 32, 40, 67, 801, 1024}) walk_unknowns(M);
    for (int M : {1, 2, 10, 11, 25, 32, 40, 67}) walk_carve({M}, 120, 600, 4, true);
    walk_carve({1, 25, 10}, 153, 424, 4, true);
    walk_carve({0, 3}, 0, 0, 1, true);
    walk_carve({1024, 1024}, 4096, 40000, 8, false);
    for (int n : {1, 6, NRG_B - 1, NRG_B, NRG_B + 1, 3 * NRG_B + 5}) walk_factor({n});
    walk_factor({NRG_B + 1, 6, 3 * NRG_B + 5});
    walk_factor({0, 6 * 67, 6 * 40});
    std::printf("nonrigid_gn_index_check: ok (%lld assembly elements, %lld update tiles walked)\n", g_elems, g_tiles);
    return 0;
}
