// Host build of the p-value routine of csrc/tonal_anova.hip (f_survival is __host__ __device__): reads "F dfb dfw" lines,
// prints p with 17 digits.  Built and driven by scripts/check_f_survival.py.
#include "../decode_tonal_langauge_amd/csrc/tonal_anova.hip"
namespace tl { void set_error(const char*, ...) {} }
int main() {
  double F, dfb, dfw;
  while (scanf("%lf %lf %lf", &F, &dfb, &dfw) == 3) printf("%.17g\n", tl::f_survival(F, dfb, dfw));
  return 0;
}
