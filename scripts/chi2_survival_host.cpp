// Host build of the chi-square tail of csrc/tonal_anova.hip (chi2_survival is __host__ __device__): reads "H df" lines, prints p
// with 17 digits.  Built and driven by scripts/check_chi2_survival.py.
#include "../decode_tonal_langauge_amd/csrc/tonal_anova.hip"
namespace tl { void set_error(const char*, ...) {} }
int main() {
  double H, df;
  while (scanf("%lf %lf", &H, &df) == 2) printf("%.17g\n", tl::chi2_survival(H, df));
  return 0;
}
