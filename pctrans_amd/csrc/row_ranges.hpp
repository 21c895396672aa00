// The rows of the query-contrast ("re-id") loss by image, for reid_dice.hip and reid_query.hip.  The two feed the same loss and
// must agree on which rows count: image_start[n] .. image_start[n + 1] are the rows of image n among key[0 .. I), and every
// rule that guards a bad image_start or key is stated here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

namespace pct {

// the rows [first, first + rows) of image n, clamped so that they index key[0 .. I) and at most Q of them count: first is
// clamped to [0, I] before it indexes anything, rows to [0, min(I - first, Q)]
__device__ __forceinline__ void image_rows(const int *__restrict__ image_start, const int n, const int I, const int Q, int &first,
                                           int &rows)
{
  const long long a = image_start[n], b = image_start[n + 1];
  const long long f = a < 0 ? 0 : (a > I ? I : a);
  long long r = b - f;
  const long long cap = (long long)(I - f) < Q ? (long long)(I - f) : Q;
  r = r < 0 ? 0 : (r > cap ? cap : r);
  first = (int)f;
  rows = (int)r;
}

// the image of row i: the largest n in [0, N) with image_start[n] <= i (empty images in front of it skipped)
__device__ __forceinline__ int image_of(const int *__restrict__ image_start, const int N, const int i)
{
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (image_start[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// row i counts: it lies inside its image's clamped range and its key is a query.  -> the image, or -1
__device__ __forceinline__ int row_image(const int *__restrict__ image_start, const int *__restrict__ key, const int N, const int I,
                                         const int Q, const int i)
{
  const int n = image_of(image_start, N, i);
  int first, rows;
  image_rows(image_start, n, I, Q, first, rows);
  if (i < first || i >= first + rows) return -1;
  return (unsigned)key[i] < (unsigned)Q ? n : -1;
}

}  // namespace pct
