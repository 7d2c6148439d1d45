// genc_host.cpp -- general GF(2) encoder for any ldpc_code: builds, by bit-packed
// elimination of H, the matrix P with parity = P * info, and encodes on the
// host.  (The reference has no encoder for these codes: its GenericEncoder,
// code/x86/CEncoder/GenericEncoder.cpp:38-78, is IRA-only.)
//
// The result is defined without reference to the elimination order:
//   parity positions: scanning columns N-1 .. 0, a column is a parity position
//     iff it is linearly independent of the parity columns chosen before it
//     (rank of them);
//   information positions: the K = N - M lowest remaining columns, ascending;
//   forced zeros: the other M - rank free columns (rank < M only);
//   the parity bits are the unique solution of H x = 0 given the free columns.
// Reducing H to reduced row-echelon form with the columns taken from N-1 down
// yields exactly that: its pivot columns are the parity positions, and pivot
// row r reads  x[pivot r] = XOR of x[c] over the free columns c set in row r.
//
// A code built from an Annex-B table needs none of this: its staircase columns
// K .. N-1 are lower bidiagonal, hence independent, hence the canonical parity
// positions, and the unique solution is what ldpc_dvbs2_encode computes.
#include <algorithm>
#include <cstring>
#include <new>

#include "genc.h"

uint64_t genc_code_hash(const ldpc_code *h)
{
    uint64_t x = 0xcbf29ce484222325ull;
    auto mix = [&](uint64_t v) { x = (x ^ v) * 0x100000001b3ull; };
    mix((uint64_t)h->n);
    mix((uint64_t)h->m);
    for (int d : h->group_deg) mix((uint64_t)d);
    for (int c : h->group_cnt) mix((uint64_t)c);
    for (uint32_t v : h->edge_var) mix(v);
    return x;
}

namespace {

// RREF of the dense rows (nw words each), columns from n-1 down; pivot_col[r]
// = pivot column of row r or -1.  Only rows holding the pivot bit are touched.
int eliminate(std::vector<uint64_t> &a, int m, int n, size_t nw, std::vector<int> &pivot_col)
{
    pivot_col.assign(m, -1);
    int rank = 0;
    for (int c = n - 1; c >= 0 && rank < m; c--) {
        const size_t w = (size_t)c >> 6;
        const uint64_t bit = 1ull << (c & 63);
        int pr = -1;
        for (int r = 0; r < m; r++)
            if (pivot_col[r] < 0 && (a[r * nw + w] & bit)) {
                pr = r;
                break;
            }
        if (pr < 0) continue;
        pivot_col[pr] = c;
        rank++;
        // no row holds a bit in a pivot column above c, and the free columns
        // above c keep whatever they have: every word of the row takes part
        const uint64_t *src = &a[pr * nw];
        for (int r = 0; r < m; r++) {
            if (r == pr || !(a[r * nw + w] & bit)) continue;
            uint64_t *dst = &a[r * nw];
            for (size_t i = 0; i < nw; i++) dst[i] ^= src[i];
        }
    }
    return rank;
}

}  // namespace

extern "C" int ldpc_encoder_create(const ldpc_code *h, ldpc_encoder **out)
{
    if (!out) return ldpc_set_error(LDPC_EINVAL, "encoder: out is NULL");
    *out = nullptr;
    if (!h) return ldpc_set_error(LDPC_EINVAL, "encoder: code is NULL");
    const int n = h->n, m = h->m, k = n - m;
    if (k <= 0) return ldpc_set_error(LDPC_EUNSUPPORTED, "encoder: code %dx%d has no information bits", n, m);
    auto *e = new (std::nothrow) ldpc_encoder();
    if (!e) return ldpc_set_error(LDPC_ENOMEM, "encoder");
    e->code = h;
    e->code_hash = genc_code_hash(h);
    e->n = n;
    e->m = m;
    e->k = k;
    try {
        if (h->dvbs2_q > 0) {
            e->ira = true;
            e->rank = m;
            e->systematic = true;
            e->info_pos.resize(k);
            e->parity_pos.resize(m);
            for (int i = 0; i < k; i++) e->info_pos[i] = i;
            for (int j = 0; j < m; j++) e->parity_pos[j] = k + j;
            *out = e;
            return LDPC_OK;
        }
        const size_t nw = ((size_t)n + 63) / 64;
        if ((size_t)m * nw * 8 > kGencMaxDenseBytes) {
            delete e;
            return ldpc_set_error(LDPC_EUNSUPPORTED, "encoder: the dense %d x %d bit matrix takes %zu bytes, the "
                                  "elimination is capped at %zu", m, n, (size_t)m * nw * 8, kGencMaxDenseBytes);
        }
        std::vector<uint64_t> a((size_t)m * nw, 0);
        for (int r = 0; r < m; r++) {
            const uint32_t *v = &h->edge_var[h->check_start[r]];
            for (int t = 0; t < h->check_deg[r]; t++) a[r * nw + (v[t] >> 6)] ^= 1ull << (v[t] & 63);
        }
        std::vector<int> pivot_col;
        e->rank = eliminate(a, m, n, nw, pivot_col);

        std::vector<uint8_t> is_parity(n, 0);
        std::vector<int> rows;   // pivot rows, by ascending pivot column
        for (int r = 0; r < m; r++)
            if (pivot_col[r] >= 0) {
                is_parity[pivot_col[r]] = 1;
                rows.push_back(r);
            }
        std::sort(rows.begin(), rows.end(), [&](int x, int y) { return pivot_col[x] < pivot_col[y]; });
        for (int c = 0; c < n; c++) {
            if (is_parity[c]) e->parity_pos.push_back(c);
            else if ((int)e->info_pos.size() < k) e->info_pos.push_back(c);
            else e->forced_pos.push_back(c);
        }
        e->systematic = e->info_pos[k - 1] == k - 1;

        e->kw = (k + 63) / 64;
        e->stride = (e->rank + kGencCols - 1) / kGencCols * kGencCols;
        e->pt.assign((size_t)e->kw * e->stride, 0);
        for (int j = 0; j < e->rank; j++) {
            const uint64_t *row = &a[rows[j] * nw];
            for (int i = 0; i < k; i++) {
                const int c = e->info_pos[i];
                if (row[c >> 6] >> (c & 63) & 1) e->pt[(size_t)(i >> 6) * e->stride + j] |= 1ull << (i & 63);
            }
        }
    } catch (const std::bad_alloc &) {
        delete e;
        return ldpc_set_error(LDPC_ENOMEM, "encoder: %dx%d elimination", n, m);
    }
    *out = e;
    return LDPC_OK;
}

extern "C" void ldpc_encoder_destroy(ldpc_encoder *e) { delete e; }

extern "C" int ldpc_encoder_info(const ldpc_encoder *e, int *n, int *k, int *rank, int *systematic)
{
    if (!e) return ldpc_set_error(LDPC_EINVAL, "encoder is NULL");
    if (n) *n = e->n;
    if (k) *k = e->k;
    if (rank) *rank = e->rank;
    if (systematic) *systematic = e->systematic ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_encoder_positions(const ldpc_encoder *e, int32_t *info_pos, int32_t *parity_pos)
{
    if (!e) return ldpc_set_error(LDPC_EINVAL, "encoder is NULL");
    if (info_pos) memcpy(info_pos, e->info_pos.data(), sizeof(int32_t) * e->info_pos.size());
    if (parity_pos) memcpy(parity_pos, e->parity_pos.data(), sizeof(int32_t) * e->parity_pos.size());
    return LDPC_OK;
}

extern "C" int ldpc_encode(const ldpc_encoder *e, const uint8_t *info, uint8_t *codeword, int batch)
{
    if (!e || batch < 0 || (batch > 0 && (!info || !codeword))) return ldpc_set_error(LDPC_EINVAL, "encode args");
    if (e->ira) return ldpc_dvbs2_encode(e->code, info, codeword, batch);
    const int n = e->n, k = e->k, rank = e->rank, kw = e->kw;
    const size_t stride = (size_t)e->stride;
    std::vector<uint64_t> iw(kw), acc(rank);
    for (int b = 0; b < batch; b++) {
        const uint8_t *in = info + (size_t)b * k;
        uint8_t *cw = codeword + (size_t)b * n;
        std::fill(iw.begin(), iw.end(), 0);
        for (int i = 0; i < k; i++) {
            const uint64_t bit = in[i] & 1;
            iw[i >> 6] |= bit << (i & 63);
            cw[e->info_pos[i]] = (uint8_t)bit;
        }
        std::fill(acc.begin(), acc.end(), 0);
        for (int w = 0; w < kw; w++) {
            const uint64_t x = iw[w];
            if (!x) continue;
            const uint64_t *p = &e->pt[w * stride];
            for (int j = 0; j < rank; j++) acc[j] ^= p[j] & x;
        }
        for (int j = 0; j < rank; j++) cw[e->parity_pos[j]] = (uint8_t)(__builtin_popcountll(acc[j]) & 1);
        for (int32_t c : e->forced_pos) cw[c] = 0;
    }
    return LDPC_OK;
}
